"""sqr.conv.dgrad_route: which of the backward-data routes a conv's input gradient takes, and what the
executor in Conv2dFn.backward has to do around it.  The chooser launches nothing and loads no library:
CPU tensors stand for the operands.  Pure host logic, no GPU.

Default conv: N, C, H, W = 2, 64, 16, 16, K = 64, 3x3 / stride 1 / pad 1, bf16, channels-last."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sq-recovery_amd"))

from sqr import conv as sc  # noqa: E402
from sqr.bn import Deferred  # noqa: E402

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
CL = torch.channels_last
ACC_ROUTES = ("acc", "acc_masked", "acc_s2")


def _desc(C=64, H=16, W=16, K=64, R=3, stride=1, pad=1, dt=BF16):
    return sc._desc(2, C, H, W, K, R, R, stride, pad, dt)


def _t(shape=(2, 64, 16, 16), dtype=BF16, cl=True):
    t = torch.zeros(shape, dtype=dtype)
    return t.contiguous(memory_format=CL) if cl else t


def _link(dtype=BF16):
    link = sc.BnBackwardLink()
    link.x, link.mask, link.mean = _t(dtype=dtype), torch.zeros(2 * 16 * 16 * 8, dtype=torch.uint8), torch.zeros(64)
    assert link.ready()
    return link


def _deferred(link):
    """A Deferred that is the link's, nothing written yet: (deferred, the conv's saved input = its y)."""
    pend = Deferred(link.x, torch.zeros(128), link.mask, _t())
    link.deferred = pend
    return pend, pend.y


def _masked(shape=(2, 64, 16, 16), dtype=BF16, cl=True):
    return sc.MaskedGrad(_t(shape, dtype, cl), torch.zeros(2 * 16 * 16 * 8, dtype=torch.uint8))


def _join(acc_done=False):
    j = sc.ResidualJoin()
    j.acc_done = acc_done
    return j


def _route(d=None, addend=None, link=None, deferred=None, xin=None, join=None, role=None, dt=BF16):
    r = sc.dgrad_route(d if d is not None else _desc(), dt, addend, link, deferred, xin, join, role)
    assert r.whole == (r.name in ACC_ROUTES)  # dx is the whole gradient of x exactly on the acc* routes
    return r


def _is(r, name, expand=False, materialize=False, add=False):
    assert (r.name, r.expand, r.materialize, r.add) == (name, expand, materialize, add), r
    assert r.whole == (name in ACC_ROUTES)


def test_nothing_attached_is_plain():
    _is(_route(), "plain")
    _is(_route(join=_join(), role="acc"), "plain")  # conv1 ran first: nothing deposited


def test_ready_link_is_bn():
    _is(_route(link=_link()), "bn")
    link = sc.BnBackwardLink()  # the BatchNorm's forward filled nothing
    _is(_route(link=link), "plain")


def test_link_with_unwritten_deferred_is_bn_act():
    link = _link()
    pend, xin = _deferred(link)
    _is(_route(link=link, deferred=pend, xin=xin), "bn_act")
    _is(_route(link=link, deferred=pend, xin=None), "bn_act")  # no weight gradient: no activation wanted


def test_link_with_written_deferred_is_bn_after_materialize():
    link = _link()
    pend, xin = _deferred(link)
    pend.y_written = True
    _is(_route(link=link, deferred=pend, xin=xin), "bn", materialize=True)


def test_deferred_of_another_link_or_another_input_is_bn_after_materialize():
    link = _link()
    pend, xin = _deferred(link)
    link.deferred = None
    _is(_route(link=link, deferred=pend, xin=xin), "bn", materialize=True)
    link.deferred = pend
    _is(_route(link=link, deferred=pend, xin=_t()), "bn", materialize=True)  # xin is not deferred.y


@pytest.mark.parametrize("addend, name", [(_t(), "acc"), (_masked(), "acc_masked")], ids=["tensor", "masked"])
def test_addend_wins_over_a_ready_link(addend, name):
    link = _link()
    pend, xin = _deferred(link)
    _is(_route(addend=addend, link=link, deferred=pend, xin=xin, join=_join(), role="acc"), name)
    _is(_route(addend=addend, link=_link(), join=_join(), role="acc"), name)


def test_addend_that_does_not_fit_still_disables_the_link():
    _is(_route(addend=_t(dtype=F16), link=_link(), join=_join(), role="acc"), "plain", add=True)


def test_link_of_another_dtype_is_plain():
    _is(_route(link=_link(F32)), "plain")
    link = _link(F32)
    pend, xin = _deferred(link)
    _is(_route(link=link, deferred=pend, xin=xin), "plain")


def test_fitting_masked_grad_is_acc_masked():
    _is(_route(addend=_masked(), join=_join(), role="acc"), "acc_masked")


@pytest.mark.parametrize("d, addend", [
    (_desc(R=1, pad=0), _masked()),
    (_desc(), _masked(dtype=F16)),
    (_desc(), _masked(cl=False)),
    (_desc(), _masked(shape=(2, 64, 16, 8))),
    (_desc(stride=2), _masked()),
], ids=["1x1", "fp16_vs_bf16", "not_channels_last", "other_shape", "stride2"])
def test_masked_grad_that_does_not_fit_is_expanded_for_acc(d, addend):
    _is(_route(d=d, addend=addend, join=_join(), role="acc"), "acc", expand=True)


def _compact(H=16, W=16, tshape=(2, 64, 8, 8), dtype=BF16, cl=True):
    return sc.CompactS2(_t(tshape, dtype, cl), (2, 64, H, W))


def test_fitting_compact_s2_is_acc_s2():
    _is(_route(d=_desc(stride=2), addend=_compact(), join=_join(), role="acc"), "acc_s2")


@pytest.mark.parametrize("d, addend", [
    (_desc(H=15, stride=2), _compact(H=15, tshape=(2, 64, 7, 8))),
    (_desc(W=15, stride=2), _compact(W=15, tshape=(2, 64, 8, 7))),
    (_desc(stride=2), _compact(tshape=(2, 64, 8, 4))),
    (_desc(stride=2), _compact(dtype=F16)),
    (_desc(stride=2), _compact(cl=False)),
    (_desc(stride=1), _compact()),
], ids=["odd_H", "odd_W", "wrong_compact_shape", "fp16_vs_bf16", "not_channels_last", "stride1"])
def test_compact_s2_that_does_not_fit_is_expanded_for_acc(d, addend):
    _is(_route(d=d, addend=addend, join=_join(), role="acc"), "acc", expand=True)


def test_tensor_addend():
    j = dict(join=_join(), role="acc")
    _is(_route(addend=_t(), **j), "acc")
    _is(_route(addend=_t(dtype=F16), **j), "plain", add=True)
    _is(_route(addend=_t(dtype=F32), **j), "plain", add=True)
    _is(_route(addend=_t(cl=False), **j), "plain", add=True)
    _is(_route(addend=_t(shape=(2, 64, 16, 8)), **j), "plain", add=True)
    _is(_route(d=_desc(R=1, pad=0), addend=_t(), **j), "acc")  # any conv geometry: the entry has its own fallback


def test_expanded_addends_choose_again_as_tensors():
    """What Conv2dFn.backward does after full(): the tensor goes through acc, or plain and a Python add."""
    j = dict(join=_join(), role="acc")
    _is(_route(addend=_masked().full(), **j), "acc")                       # refused by the C entry, or 1x1
    _is(_route(addend=_masked(dtype=F16).full(), **j), "plain", add=True)  # still fp16 against bf16
    _is(_route(d=_desc(H=15, stride=2), addend=_compact(H=15, tshape=(2, 64, 8, 8)).full(), **j), "acc")


def _ds(H=16, W=16, C=64):
    return _desc(C=C, H=H, W=W, K=128, R=1, stride=2, pad=0)


def test_downsample_conv_deposits_compact():
    _is(_route(d=_ds(), join=_join(), role="dep"), "compact")
    _is(_route(d=_ds(C=8), join=_join(), role="dep"), "compact")


@pytest.mark.parametrize("d, kw", [
    (_ds(), dict(join=_join(acc_done=True), role="dep")),   # conv1's backward already ran
    (_ds(W=15), dict(join=_join(), role="dep")),
    (_ds(H=15), dict(join=_join(), role="dep")),
    (_ds(), dict(join=_join(), role="acc")),
    (_ds(), dict()),
    (_desc(K=128, R=1, stride=1, pad=0), dict(join=_join(), role="dep")),
    (_desc(K=128, R=3, stride=2, pad=1), dict(join=_join(), role="dep")),
    (_desc(K=128, R=1, stride=2, pad=1), dict(join=_join(), role="dep")),
], ids=["acc_done", "odd_W", "odd_H", "role_acc", "no_join", "stride1", "3x3", "pad1"])
def test_downsample_conv_that_cannot_deposit_compact_is_plain(d, kw):
    _is(_route(d=d, **kw), "plain")


def test_link_wins_over_compact():
    _is(_route(d=_ds(), link=_link(), join=_join(), role="dep"), "bn")


def test_whole_gradient_exactly_on_the_acc_routes():
    j = dict(join=_join(), role="acc")
    link = _link()
    pend, xin = _deferred(link)
    seen = {}
    for r in (_route(), _route(link=_link()), _route(link=link, deferred=pend, xin=xin), _route(addend=_t(), **j),
              _route(addend=_masked(), **j), _route(d=_desc(stride=2), addend=_compact(), **j),
              _route(d=_ds(), join=_join(), role="dep"), _route(addend=_t(dtype=F16), **j)):
        seen.setdefault(r.name, set()).add(r.whole)
    assert seen == {"plain": {False}, "bn": {False}, "bn_act": {False}, "compact": {False},
                    "acc": {True}, "acc_masked": {True}, "acc_s2": {True}}

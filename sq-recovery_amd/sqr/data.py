"""Host -> device batch prefetch for the h5 data path.

The reference feeds train.py from a torch DataLoader over H5Dataset (torch/train.py:24-40,
torch/classes.py:32-101) and copies each batch to the GPU synchronously at the top of the step.
Here the DataLoader's worker processes decode into pinned host memory (pin_memory=True) and
DevicePrefetcher copies batch i+1 to the device on a side HIP stream while batch i trains: the
copy engine and the compute stream overlap, and the compute stream waits only on an event.  On a
CPU device it is a plain pass-through.

OnlineSource needs no dataset at all: it draws each batch's labels on the device with a counter-based
sampler (sqr_sq_sample: sample i of substream s under seed k is a pure function of (k, s, i)) and renders
them there (sqr_scan_render / sqr_implicit_render).  The stream position lives in device memory, read by
the sampler and moved by a one-thread launch (sqr_sq_stream_advance), so next() can be captured in a HIP
graph and every replay draws new samples.
"""
import torch

from . import cpu as _cpu
from ._lib import check, lib, ptr, stream_ptr

_MASK64 = 2 ** 64 - 1


def _as_i64(v):
    """The int64 with the bit pattern of the uint64 v (torch holds the position as int64)."""
    v = int(v) & _MASK64
    return v - 2 ** 64 if v >= 2 ** 63 else v


def sq_sample(position, seed, substream, offset, B, params=None, raw=None):
    """sqr_sq_sample on the current stream: rows *position + offset + b of (seed, substream) into `params`
    ([B,12] f32, allocated when None) and, when given, their words into `raw` ([B,12] int32 holding the
    uint32 bit patterns).  position: a one-element CUDA int64 tensor (read as uint64).  Returns params."""
    if not position.is_cuda or position.dtype != torch.int64 or position.numel() != 1:
        raise ValueError("position must be a one-element CUDA int64 tensor")
    if params is None:
        params = torch.empty(B, 12, dtype=torch.float32, device=position.device)
    for t, dt, what in ((params, torch.float32, "params"), (raw, torch.int32, "raw")):
        if t is not None and (t.dtype != dt or t.device != position.device or not t.is_contiguous()
                              or t.numel() < B * 12):
            raise ValueError("%s must be a contiguous %s tensor of [%d,12] on %s" % (what, dt, B, position.device))
    check(lib().sqr_sq_sample(ptr(position), int(seed) & _MASK64, int(substream) & 0xFFFFFFFF, int(offset) & _MASK64,
                              int(B), ptr(params), ptr(raw), stream_ptr(position.device)), "sqr_sq_sample")
    return params


def stream_advance(position, stride):
    """sqr_sq_stream_advance on the current stream: *position += stride (modulo 2^64)."""
    if not position.is_cuda or position.dtype != torch.int64 or position.numel() != 1:
        raise ValueError("position must be a one-element CUDA int64 tensor")
    check(lib().sqr_sq_stream_advance(ptr(position), int(stride) & _MASK64, stream_ptr(position.device)),
          "sqr_sq_stream_advance")


class OnlineSource:
    """An endless stream of fresh (images [B,1,size,size] f32, labels [B,12] f32) batches made on `device`.

    next() runs the sampler with offset = rank * B, the advance with stride = world * B and the renderer
    ("scanner": sqr_scan_render with `levels`; "soft": sqr_implicit_render with tau, sharpness) on the current
    stream, into static buffers it owns, and returns them: no host wait, no allocation, capturable.  The
    ranks of a data-parallel job together consume one contiguous stream, so sample i is the same image
    whatever the batch size and the number of GPUs.  On a CPU device the sampler is sqr.cpu.sq_sample and
    the renderers are sqr.cpu.scan_render / render (plumbing for small sizes)."""

    def __init__(self, batch, device, size=256, seed=0, substream=0, rank=0, world=1, render="scanner", levels=255,
                 tau=1.5, sharpness=260):
        if render not in ("soft", "scanner"):
            raise ValueError("render must be 'soft' or 'scanner', got %r" % (render,))
        if not 1 <= int(batch) <= 65535:
            raise ValueError("batch=%d out of range [1,65535]" % batch)
        if not 0 <= int(rank) < int(world):
            raise ValueError("rank %d outside world %d" % (rank, world))
        self.batch, self.size, self.device = int(batch), int(size), torch.device(device)
        self.seed, self.substream = int(seed) & _MASK64, int(substream) & 0xFFFFFFFF
        self.rank, self.world = int(rank), int(world)
        self.render, self.levels, self.tau, self.sharpness = render, int(levels), float(tau), float(sharpness)
        self.cuda = self.device.type == "cuda"
        self._pos = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.images = torch.zeros(self.batch, 1, self.size, self.size, dtype=torch.float32, device=self.device)
        self.labels = torch.zeros(self.batch, 12, dtype=torch.float32, device=self.device)

    def next(self):
        B = self.batch
        if not self.cuda:
            pos = int(self._pos.item()) & _MASK64
            self.labels.copy_(torch.from_numpy(_cpu.sq_sample(pos + self.rank * B, B, self.seed, self.substream)))
            self._pos.fill_(_as_i64(pos + self.world * B))
            if self.render == "scanner":
                img = _cpu.scan_render(self.labels, self.size, self.levels)
            else:
                img = _cpu.render(self.labels, self.size, self.tau, self.sharpness)
            self.images[:, 0] = img.to(torch.float32)
            return self.images, self.labels
        sq_sample(self._pos, self.seed, self.substream, self.rank * B, B, self.labels)
        stream_advance(self._pos, self.world * B)
        L, st = lib(), stream_ptr(self.device)
        if self.render == "scanner":
            check(L.sqr_scan_render(ptr(self.labels), B, self.size, self.levels, ptr(self.images), st),
                  "sqr_scan_render")
        else:
            check(L.sqr_implicit_render(ptr(self.labels), B, self.size, self.tau, self.sharpness, ptr(self.images),
                                        st), "sqr_implicit_render")
        return self.images, self.labels

    def seek(self, pos):
        """Set the stream position (the sample number the next round of batches starts at)."""
        self._pos.fill_(_as_i64(pos))

    def position(self):
        """The current position (a host read: waits for the work queued on the device)."""
        return int(self._pos.item()) & _MASK64

    def state_dict(self):
        return {"seed": self.seed, "substream": self.substream, "position": self.position()}

    def load_state_dict(self, state):
        self.seed, self.substream = int(state["seed"]) & _MASK64, int(state["substream"]) & 0xFFFFFFFF
        self.seek(state["position"])


def _to(obj, device):
    if torch.is_tensor(obj):
        return obj.to(device, non_blocking=True)
    if isinstance(obj, (list, tuple)):
        return type(obj)(_to(o, device) for o in obj)
    return obj


def _record(obj, stream):
    if torch.is_tensor(obj):
        obj.record_stream(stream)
    elif isinstance(obj, (list, tuple)):
        for o in obj:
            _record(o, stream)


class DevicePrefetcher:
    """Iterate `loader` (batches of tensors / tuples of tensors) with every batch already on
    `device`: batch i+1's host->device copy runs on a side stream during batch i."""

    def __init__(self, loader, device):
        self.loader = loader
        self.device = torch.device(device)
        self.cuda = self.device.type == "cuda"

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        if not self.cuda:
            yield from self.loader
            return
        side = torch.cuda.Stream(device=self.device)
        it = iter(self.loader)

        def stage():
            try:
                host = next(it)
            except StopIteration:
                return None
            with torch.cuda.stream(side):
                dev = _to(host, self.device)
                ev = torch.cuda.Event()
                ev.record(side)
            return dev, ev

        nxt = stage()
        while nxt is not None:
            dev, ev = nxt
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(ev)
            _record(dev, cur)  # the caching allocator must not recycle it before the compute stream is done
            nxt = stage()      # next copy overlaps this batch's compute
            yield dev

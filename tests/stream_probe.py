"""Test helper of tests/test_gpu_streams.py: what include/jpezy_hip.h promises of every *_dev entry point about streams -- asynchronous on
the caller's stream, in that stream's order, capturable -- turned into three procedures over a Probe, which is one call of one entry with
two inputs A and B of one size, layout and set of tables (so that going from A to B uploads nothing).

stream_order   the call is handed a side stream on which a delay and the copy that turns the input from A into B are still pending.  It
               must return while the delay runs (no wait for the stream or the device), and the output must be B's: a launch on any other
               stream runs during the delay, reads A (or the scratch of the warm call) and leaves A's bytes.
wrong_stream   the control: the same sandwich with the call on a second, idle stream.  The output must be A's, a stale read by
               construction -- the procedure above can fail.
capture_replay one call captured on a side stream into a graph of one stream without branches, replayed on A, B, A.

Outputs are pre-filled with a marker byte, are longer than the entry needs and are compared as a whole.  The expectations are the
caller's (the numpy models and the oracle); nothing here is compared with another call of the entry under test."""
import time

import numpy as np
import pytest

FILL = 0xA5
DEVICE_FACTOR, HOST_FACTOR = 50, 100      # the delay against the call's device and host time: margins for a shared machine, not tuned
MAX_DELAY_MS = 500.0


class Delay:
    """a kernel that keeps a stream busy for a given time: torch.cuda._sleep, calibrated once with events; where torch has none, a chain of
    elementwise operations on one large tensor"""

    def __init__(self, torch, device):
        self.torch = torch
        self.sleep = getattr(torch.cuda, "_sleep", None)
        self.largest_ms = 0.0
        if self.sleep is None:
            self.big = torch.zeros(1 << 26, dtype=torch.float32, device=device)
        unit = 1 << 16 if self.sleep is not None else 1
        self._run(unit)                                            # (code load)
        torch.cuda.synchronize()
        while True:                                                # grow until the timed run is long against the events' resolution
            ms = self._timed(unit)
            if ms >= 2.0 or unit >= 1 << 40:
                break
            unit *= 8 if self.sleep is not None else 2
        self.units_per_ms = unit / ms

    def _run(self, units):
        if self.sleep is not None:
            self.sleep(int(units))
        else:
            for _ in range(int(units)):
                self.big.add_(1.0)

    def _timed(self, units):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self._run(units)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def queue(self, ms):
        """on the current stream"""
        self.largest_ms = max(self.largest_ms, ms)
        self._run(max(1, round(ms * self.units_per_ms)))

    def describe(self):
        what = "cycles of torch.cuda._sleep" if self.sleep is not None else "elementwise operations"
        return f"{self.units_per_ms:.0f} {what} per millisecond, largest delay used {self.largest_ms:.2f} ms"


class Probe:
    """one call of one entry.  inputs: [(device tensor the entry reads, A, B)] with A and B numpy arrays of its shape and dtype; outputs:
    device tensors (contiguous, any dtype); call(stream): the entry on that hipStream_t (an integer); expect: {"A" | "B": one (bytes, mask)
    per output} -- the whole buffer as uint8, mask None or a bool array of the bytes that are defined (a .jpg slot behind its file is not)"""

    def __init__(self, torch, name, inputs, outputs, call, expect):
        self.torch, self.name, self.outputs, self.call, self.expect = torch, name, outputs, call, expect
        self.inputs = [(d, {"A": torch.from_numpy(np.array(a)).to(d.device), "B": torch.from_numpy(np.array(b)).to(d.device)}) for d, a, b in inputs]
        for d, src in self.inputs:
            assert src["A"].shape == d.shape and src["A"].dtype == d.dtype and not torch.equal(src["A"], src["B"]), name
        for (wa, ma), (wb, mb) in zip(expect["A"], expect["B"]):
            both = np.ones(wa.size, bool) if ma is None and mb is None else (np.ones(wa.size, bool) if ma is None else ma) & (np.ones(wb.size, bool) if mb is None else mb)
            assert wa.dtype == np.uint8 and wa.shape == wb.shape and (wa[both] != wb[both]).any(), (name, "the expectations for A and B do not differ")
        for o, (w, _) in zip(outputs, expect["A"]):
            assert o.is_contiguous() and o.numel() * o.element_size() == w.size, (name, "expectation and output differ in size")
            assert (w == FILL).any(), (name, "the output is no longer than the entry needs")

    def load(self, which):
        """on the current stream"""
        for d, src in self.inputs:
            d.copy_(src[which])

    def refill(self):
        for o in self.outputs:
            o.view(self.torch.uint8).fill_(FILL)

    def compare(self, which, what):
        for k, (o, (want, mask)) in enumerate(zip(self.outputs, self.expect[which])):
            got = o.view(self.torch.uint8).reshape(-1).cpu().numpy()
            diff = got != want if mask is None else (got != want) & mask
            bad = np.nonzero(diff)[0]
            if bad.size:
                other = self.expect["B" if which == "A" else "A"][k]
                omask = np.ones(got.size, bool) if other[1] is None else other[1]
                stale = bool((got[omask] == other[0][omask]).all())
                pytest.fail(f"{self.name}: {what}: output {k} is not the expectation for {which}: {bad.size} bytes differ, the first at {int(bad[0])} "
                            f"(got {int(got[bad[0]])}, want {int(want[bad[0]])})" + ("; it IS the expectation for the other input" if stale else ""))


def _default_stream(torch):
    return torch.cuda.current_stream().cuda_stream


def warm_and_measure(torch, p):
    """the entry on the default stream with input A, twice: the first call uploads the tables and the header, grows every scratch buffer and
    loads the kernels' code; the second is timed and compared with the expectation for A.  Device time: between two events around the
    call.  Host time: the copy of the input and the call, which is what the sandwich issues between the delay and its look at the
    event.  -> (device ms, host ms)"""
    p.load("A")
    p.refill()
    torch.cuda.synchronize()
    p.call(_default_stream(torch))
    torch.cuda.synchronize()
    p.refill()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    p.load("A")
    e0.record()
    p.call(_default_stream(torch))
    e1.record()
    host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    p.compare("A", "warm call on the default stream")
    return e0.elapsed_time(e1), host_ms


def _sandwich(torch, delay, p, on_idle_stream):
    dev_ms, host_ms = warm_and_measure(torch, p)
    ms = max(DEVICE_FACTOR * dev_ms, HOST_FACTOR * host_ms)
    print(f"stream probe: {p.name}: warm call {dev_ms * 1e3:.1f} us on the device, {host_ms * 1e3:.1f} us on the host; delay {ms:.2f} ms")
    if ms > MAX_DELAY_MS:
        pytest.fail(f"{p.name}: a delay of {ms:.1f} ms would be needed (device {dev_ms:.3f} ms, host {host_ms:.3f} ms): no case may need "
                    f"more than {MAX_DELAY_MS:.0f} ms at these shapes")
    p.load("A")
    p.refill()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    ev = torch.cuda.Event()
    with torch.cuda.stream(s):
        delay.queue(ms)
        ev.record()
        p.load("B")
    print(f"stream probe: {delay.describe()}")
    if not on_idle_stream:
        p.call(s.cuda_stream)
        returned_early = not ev.query()
        s.synchronize()
        assert returned_early, (f"{p.name}: the delay queued in front of the call on its own stream had ended when the call returned: the call "
                                f"waited for the stream or the device (or {ms:.2f} ms were too short)")
        p.compare("B", "call on a side stream behind a delay and the copy of input B")
        return
    s2 = torch.cuda.Stream()
    p.call(s2.cuda_stream)
    s2.synchronize()
    still = not ev.query()
    s.synchronize()
    if not still:
        pytest.fail("delay too short for the control")
    p.compare("A", "control: call on an idle stream while the copy of input B waits behind the delay")


def stream_order(torch, delay, p):
    _sandwich(torch, delay, p, False)


def wrong_stream(torch, delay, p):
    _sandwich(torch, delay, p, True)


def capture_replay(torch, p):
    """a warm call outside the capture, one call captured on a side stream, three replays on A, B, A"""
    p.load("A")
    p.refill()
    torch.cuda.synchronize()
    p.call(_default_stream(torch))
    torch.cuda.synchronize()
    p.compare("A", "warm call on the default stream")
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    p.refill()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            p.call(s.cuda_stream)
    for k, which in enumerate("ABA"):
        p.load(which)
        p.refill()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        p.compare(which, f"replay {k} of the captured call")


# ---- expectations: whole buffers of marker bytes with the entry's bytes written over them ---------------------------------------------
def marker(nbytes):
    return np.full(nbytes, FILL, np.uint8)


def planes_buffers(frames, stride, tail):
    """frames: [frame][plane] arrays of one size -> three buffers of len(frames) * stride + tail bytes, frame f's plane at f * stride"""
    out = [marker(len(frames) * stride + tail) for _ in range(3)]
    for f, planes in enumerate(frames):
        for k in range(3):
            flat = np.asarray(planes[k], np.uint8).reshape(-1)
            out[k][f * stride:f * stride + flat.size] = flat
    return [(o, None) for o in out]


def packed_buffer(images, row_stride, frame_stride, tail):
    """images: [frame] arrays (h, w, bytes) -> one buffer, rows row_stride apart, frames frame_stride apart"""
    out = marker(len(images) * frame_stride + tail)
    for f, img in enumerate(images):
        h, w, nb = img.shape
        for y in range(h):
            at = f * frame_stride + y * row_stride
            out[at:at + w * nb] = img[y].reshape(-1)
    return [(out, None)]

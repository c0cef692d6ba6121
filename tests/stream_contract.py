"""The delayed-stream harness of test_stream_contract.py: one device entry called on a side stream whose inputs arrive late.

Every device input of the entry is allocated up front and holds a DECOY, another valid input of the same size.  On a non-blocking
side stream s are queued, in this order: a delay (torch.cuda._sleep, calibrated once per session to DELAY_MS), device-to-device
copies of the real inputs over the decoys, and the sentinel fill of the outputs and of the guard bytes behind them.  Then the entry
is called with s, its host arguments are overwritten with the decoy's as soon as it returns, a clone of the outputs is queued on s,
and s is synchronised.  A launch or copy the entry queues anywhere but on s runs while the delay still holds the producer back: it
reads the decoy, and whatever it writes is then covered by the sentinel fill.  A host argument read after the return is the
decoy's.  Either way the result is not the real one, byte for byte.

A run counts only when the delay it measured (events on s) is at least MIN_DELAY_MS and at least MIN_RATIO times the entry's own
time on an idle stream with the same shapes; otherwise the test fails as inconclusive.  The premise that torch's side streams are
non-blocking is checked on the HIP runtime itself (hipStreamGetFlags) for every stream the harness hands out."""
import ctypes as C

import numpy as np

SENTINEL = 0xA5
GUARD = 64                    # sentinel bytes behind every buffer
DELAY_MS = 30.0
MIN_DELAY_MS = 20.0
MAX_DELAY_MS = 400.0
MIN_RATIO = 10.0
HIP_STREAM_NON_BLOCKING = 0x01

_state = {}
TIMES = []                    # (case name, delay ms, solo ms) of every conclusive run, in order


def _torch():
    import torch
    return torch


def _hip_runtime():
    """The HIP runtime this process has loaded (torch's own), by its path in the process's map."""
    if "hip" not in _state:
        _torch().cuda.init()
        path = None
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    path = line.split()[-1]
                    break
        assert path is not None, "no HIP runtime is loaded in this process"
        lib = C.CDLL(path)
        lib.hipStreamGetFlags.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
        lib.hipStreamGetFlags.restype = C.c_int
        _state["hip"] = lib
    return _state["hip"]


def side_stream():
    """A torch side stream, after checking on the runtime that it does not synchronise with the null stream."""
    s = _torch().cuda.Stream()
    flags = C.c_uint(0)
    assert s.cuda_stream != 0
    assert _hip_runtime().hipStreamGetFlags(C.c_void_p(s.cuda_stream), C.byref(flags)) == 0
    assert flags.value & HIP_STREAM_NON_BLOCKING, "torch.cuda.Stream() is a blocking stream: the harness would see nothing"
    return s


def _sleep_ms(s, cycles):
    torch = _torch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        e0.record(s)
        torch.cuda._sleep(int(cycles))
        e1.record(s)
    s.synchronize()
    return e0.elapsed_time(e1)


def delay_cycles(ms=DELAY_MS):
    """The argument of torch.cuda._sleep that lasts `ms` here, from one measurement per session."""
    if "cycles" not in _state:
        s = side_stream()
        _sleep_ms(s, 1000)                                   # the kernel's first launch
        cycles = 1 << 16
        took = _sleep_ms(s, cycles)
        while took < 2.0 and cycles < (1 << 36):
            cycles *= 4
            took = _sleep_ms(s, cycles)
        took = min(took, _sleep_ms(s, cycles))
        assert took >= 2.0, "torch.cuda._sleep(%d) lasted %.3f ms" % (cycles, took)
        _state["cycles"] = cycles / took
        print("stream contract: torch.cuda._sleep(%d) lasted %.3f ms: %.0f cycles per ms" % (cycles, took, _state["cycles"]))
    return int(_state["cycles"] * ms)


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class Buf:
    """One device buffer of an entry.  An input has `real` and `decoy` (equal sizes); an output has `nbytes` and out=True; a
    buffer drawn into in place has all of them; scratch=True: contents irrelevant, neither filled on the stream nor compared."""

    def __init__(self, name, real=None, decoy=None, nbytes=None, out=False, scratch=False):
        self.name, self.out, self.scratch = name, out, scratch
        self.real = None if real is None else as_bytes(real).copy()
        self.decoy = None if decoy is None else as_bytes(decoy).copy()
        self.nbytes = int(nbytes) if nbytes is not None else len(self.real)
        if self.real is not None:
            assert self.decoy is not None and len(self.real) == len(self.decoy) == self.nbytes, name
        else:
            assert out or scratch, name


class Ptrs(dict):
    """buffer name -> device address; .t: buffer name -> the uint8 tensor (the buffer and the GUARD bytes behind it)"""


class Case:
    """An entry at one shape.  call(p, stream) makes the call (p: a Ptrs, stream: hipStream_t as int) and returns whatever the
    entry hands back on the host; finish(ret): for an entry whose host results come from a later wait call, made once the stream
    has been synchronised, its value replaces ret; scribble() overwrites the host arguments with the decoy's; want and
    want_decoy: output name -> the bytes the restatement expects in the whole buffer (SENTINEL where nothing is written);
    host_want: what call (or finish) must return, compared with ==, or None; host_bytes: (real, decoy) host results as bytes,
    counted with the device outputs when the decoy is held against the real output; host_key(ret): what of a host result the
    delayed run must share with the solo run; fixed: output name -> bool mask of the bytes that hold the same value whatever valid
    input of this shape the entry is given (the coefficients of blocks that only pad an image), which no decoy can change."""

    def __init__(self, name, bufs, call, want, want_decoy, scribble=None, host_want=None, finish=None, host_bytes=None, host_key=None,
                 fixed=None):
        self.name, self.bufs, self.call, self.scribble, self.host_want = name, bufs, call, scribble, host_want
        self.finish, self.host_bytes, self.host_key, self.fixed = finish, host_bytes, host_key, fixed or {}
        self.want = {k: as_bytes(v) for k, v in want.items()}
        self.want_decoy = {k: as_bytes(v) for k, v in want_decoy.items()}
        self.outs = [b for b in bufs if b.out]
        assert sorted(self.want) == sorted(self.want_decoy) == sorted(b.name for b in self.outs), name
        for b in self.outs:
            assert len(self.want[b.name]) == len(self.want_decoy[b.name]) == b.nbytes, (name, b.name)
        self.solo_ms = self.solo_out = self.solo_ret = None

    def assert_decoy_differs(self):
        """On the CPU: the decoy's output differs from the real one's in at least half of the output bytes (of those that any input
        of this shape can change, where the case names some that none can)."""
        free = [~np.asarray(self.fixed[b.name], bool) if b.name in self.fixed else np.ones(b.nbytes, bool) for b in self.outs]
        a = [self.want[b.name][m] for b, m in zip(self.outs, free)]
        d = [self.want_decoy[b.name][m] for b, m in zip(self.outs, free)]
        if self.host_bytes is not None:
            real, decoy = (as_bytes(np.frombuffer(bytes(v), np.uint8)) for v in self.host_bytes)
            n = max(len(real), len(decoy))                   # a result that is shorter differs in what it lacks
            a.append(np.concatenate([real, np.zeros(n - len(real), np.uint8)]))
            d.append(np.concatenate([decoy, np.full(n - len(decoy), 0xFF, np.uint8)]))
        a, d = np.concatenate(a), np.concatenate(d)
        assert len(a) > 0 and int((a != d).sum()) * 2 >= len(a), (self.name, int((a != d).sum()), len(a))


class Run:
    """The device side of one call of a case: allocate (decoys in place), producer (delay, real inputs, sentinels: queued on s),
    call, clone (queued on s), collect (after s was synchronised)."""

    def __init__(self, case, decoys=True):
        torch = _torch()
        self.case, self.dev, self.real_dev, self.ret = case, {}, {}, None
        for b in case.bufs:
            t = torch.empty(b.nbytes + GUARD, dtype=torch.uint8, device="cuda")
            assert t.data_ptr() % 256 == 0
            t.fill_(0xFF if b.scratch else 0)
            if b.real is not None:
                t[:b.nbytes].copy_(torch.from_numpy(b.decoy if decoys else b.real))
                self.real_dev[b.name] = torch.from_numpy(b.real).cuda()
            if not decoys:
                t[b.nbytes if b.real is not None else 0:].fill_(SENTINEL)
            self.dev[b.name] = t
        self.ptrs = Ptrs((k, t.data_ptr()) for k, t in self.dev.items())
        self.ptrs.t = self.dev
        self.events = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        self.clones = None
        torch.cuda.synchronize()

    def producer(self, s):
        torch = _torch()
        # DELAY_MS, or for an entry that itself takes milliseconds (it allocates, or waits for its own results) 15 times its time
        alone = self.case.solo_ms or 0.0
        cycles = delay_cycles(min(max(DELAY_MS, 15.0 * alone), MAX_DELAY_MS))
        with torch.cuda.stream(s):
            self.events[0].record(s)
            torch.cuda._sleep(cycles)
            self.events[1].record(s)
            for b in self.case.bufs:
                if b.real is not None:
                    self.dev[b.name][:b.nbytes].copy_(self.real_dev[b.name])
            for b in self.case.bufs:
                if not b.scratch:
                    self.dev[b.name][b.nbytes if b.real is not None else 0:].fill_(SENTINEL)

    def call(self, stream):
        self.ret = self.case.call(self.ptrs, int(stream.cuda_stream))
        return self.ret

    def scribble(self):
        if self.case.scribble is not None:
            self.case.scribble()

    def clone(self, s):
        with _torch().cuda.stream(s):
            self.clones = {b.name: self.dev[b.name].clone() for b in self.case.bufs if not b.scratch}

    def collect(self, finish=True):
        """-> output name -> bytes, after checking that the sentinels behind every buffer are still there"""
        _torch().cuda.synchronize()
        if finish and self.case.finish is not None:
            self.ret = self.case.finish(self.ret)
        got = {}
        for b in self.case.bufs:
            if b.scratch:
                continue
            flat = self.clones[b.name].cpu().numpy()
            assert (flat[b.nbytes:] == SENTINEL).all(), "%s: bytes behind %s were written to" % (self.case.name, b.name)
            if b.out:
                got[b.name] = flat[:b.nbytes]
        return got

    def delay_ms(self):
        return self.events[0].elapsed_time(self.events[1])


def solo(case):
    """The entry alone on an idle side stream with the real inputs in place: -> (outputs, host return).  The second of two calls
    is timed (events on the stream, so whatever the call itself waits for is in it); the time is kept in case.solo_ms."""
    torch = _torch()
    s = side_stream()
    for timed in (False, True):
        r = Run(case, decoys=False)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        r.call(s)
        e1.record(s)
        r.clone(s)
        s.synchronize()
    case.solo_ms = e0.elapsed_time(e1)
    case.solo_out = r.collect()
    case.solo_ret = r.ret
    return case.solo_out, case.solo_ret


def same(case, got, want, what):
    for b in case.outs:
        g, w = got[b.name], want[b.name]
        assert g.tobytes() == w.tobytes(), "%s: %s differs from %s in %d of %d bytes" % (case.name, b.name, what, int((g != w).sum()), len(w))


def conclusive(case, run):
    """The condition that keeps a run from hiding a failure; prints and records both times."""
    delay, alone = run.delay_ms(), case.solo_ms
    print("stream contract %-44s delay %7.2f ms   solo %7.3f ms" % (case.name, delay, alone))
    assert delay >= MIN_DELAY_MS and delay >= MIN_RATIO * alone, \
        "inconclusive: the delay lasted %.2f ms, the entry alone %.3f ms" % (delay, alone)
    TIMES.append((case.name, delay, alone))


def delayed(case, call_on=None):
    """One call behind the delayed producer on a fresh side stream -> (outputs, host return, the Run).  call_on: the stream the
    entry is given instead of the producer's (the controls)."""
    s = side_stream()
    r = Run(case)
    r.producer(s)
    r.call(s if call_on is None else call_on)
    r.scribble()
    r.clone(s)
    s.synchronize()
    got = r.collect()
    return got, r.ret, r


def check_entry(case):
    """The whole contract test of one case: decoy far from the real output, the solo run right, the delayed run right."""
    case.assert_decoy_differs()
    got, alone = solo(case)
    same(case, got, case.want, "the restatement (solo run)")
    if case.host_want is not None:
        assert alone == case.host_want, (case.name, "solo")
    got, ret, run = delayed(case)
    conclusive(case, run)
    same(case, got, case.want, "the restatement (delayed stream)")
    if case.host_want is not None:
        assert ret == case.host_want, (case.name, "delayed")
    if case.host_key is not None:
        assert case.host_key(ret) == case.host_key(alone), (case.name, "the delayed run's host result is not the solo run's")
    return got


def check_control(case):
    """The same sequence with the entry on a second, idle stream: the harness must see it."""
    case.assert_decoy_differs()
    solo(case)
    got, _, run = delayed(case, call_on=side_stream())
    conclusive(case, run)
    assert case.outs and any(got[b.name].tobytes() != case.want[b.name].tobytes() for b in case.outs), \
        "%s: an entry called on another stream still gave the real result" % case.name
    return got


def in_flight_together(cases):
    """One call of each case, each behind its own delayed producer on its own stream, all in flight together -> [(outputs, host result)]"""
    for c in cases:
        if c.solo_ms is None:
            solo(c)
    streams = [side_stream() for _ in cases]
    runs = [Run(c) for c in cases]
    for r, s in zip(runs, streams):
        r.producer(s)
    for r, s in zip(runs, streams):
        r.call(s)
        r.scribble()
    for r, s in zip(runs, streams):
        r.clone(s)
    for s in streams:
        s.synchronize()
    out = [(r.collect(), r.ret) for r in runs]
    for r in runs:
        conclusive(r.case, r)
    return out


def plan_reuse(first, second):
    """One plan, two calls (the cases share it): `first` behind its delayed producer on stream A and, at once, `second` on the idle
    stream B with its inputs in place.  The header's promise is that a call waits for the plan's previous call: both results must
    be right.  -> ((outputs, host result) of first, the same of second); where the host result comes from a finish call, which
    reports the plan's LAST call, the first one's is None"""
    solo(first)
    a, b = side_stream(), side_stream()
    ra, rb = Run(first), Run(second, decoys=False)
    ra.producer(a)
    ra.call(a)
    ra.scribble()
    rb.call(b)
    ra.clone(a)
    rb.clone(b)
    a.synchronize()
    b.synchronize()
    got_b = rb.collect()
    got_a = ra.collect(finish=False)
    conclusive(first, ra)
    return (got_a, None if first.finish is not None else ra.ret), (got_b, rb.ret)

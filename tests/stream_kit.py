"""What the stream-order tests share (tests/test_gpu_streams.py, tests/test_host_streams.py): a delay kernel calibrated once,
and late(): one call of the library on a SIDE stream whose inputs arrive behind that delay.

    S: [warm-up f(decoy), synchronised] [delay] [X <- real] [gate] [f(X)] ........ synchronise, compare with the reference of `real`
    default stream:                       [clone X: must still be the decoy]

X holds the decoy — valid input of the same shapes — until the delay has run out, so a kernel, memset or copy that the call
issues anywhere but on S computes the decoy's answer (or a mixture), never reads out of range, and the comparison with the
CPU reference of `real` fails.  For a call that promises not to read anything back, the gate event recorded behind the copies
must still be pending when the call returns: the host ran ahead, so nothing in the call waited for the stream.

Three conditions keep a case from passing vacuously; each is a failure, never a skip or a retry: the two references differ
(answers_differ), the control clone made on the default stream equals the decoy, and — non-blocking calls — the gate is
pending on return ("inconclusive" otherwise: the delay was too short for this host, both times are reported).

The delay of a case: max(40 ms, 20 x the host wall time of its warm-up call), at most 1 s.  A sizing rule, not a criterion.
Importing this needs no GPU."""
import time

import numpy as np

MIN_DELAY_MS = 40.0
HOST_FACTOR = 20.0
MAX_DELAY_MS = 1000.0
CALIBRATE_AT_LEAST_MS = 5.0

_calibration = {}


def delay_ms_for(host_seconds):
    """the sizing rule"""
    return min(MAX_DELAY_MS, max(MIN_DELAY_MS, HOST_FACTOR * 1e3 * host_seconds))


def _time_ms(enqueue):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    enqueue()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def calibrate(log=print):
    """-> (kind, units per millisecond) of the delay: torch.cuda._sleep cycles, or — where this torch has no _sleep — 4096^3
    float32 matmuls.  One unit count is doubled until it lasts CALIBRATE_AT_LEAST_MS; measured once per process."""
    import torch
    if "rate" in _calibration:
        return _calibration["kind"], _calibration["rate"]
    sleep = getattr(torch.cuda, "_sleep", None)
    if sleep is not None:
        kind, units, run = "sleep cycles", 1 << 18, lambda k: sleep(int(k))
    else:
        a = torch.ones((4096, 4096), dtype=torch.float32, device="cuda")
        _calibration["matmul"] = a

        def run(k):
            x = a
            for _ in range(int(k)):
                x = torch.mm(a, x)
        kind, units = "4096^3 matmuls", 1
    run(units)  # (the first launch loads the kernel)
    while True:
        ms = _time_ms(lambda: run(units))
        if ms >= CALIBRATE_AT_LEAST_MS:
            break
        units *= 2
        assert units < 1 << 44, "the delay kernel never lasts 5 ms"
    _calibration.update(kind=kind, rate=units / ms, run=run)
    log(f"stream_kit calibration: {units} {kind} = {ms:.2f} ms -> {units / ms:.1f} per ms")
    return kind, units / ms


def enqueue_delay(ms):
    """a delay of about `ms` on torch's current stream"""
    _, rate = calibrate()
    _calibration["run"](max(1, int(rate * ms)))


# ---- side streams -------------------------------------------------------------------------------------------------------------
_side = []


def _holds_back_the_default_stream(stream):
    """a delay on `stream`, then one tiny operation on the default stream: does that operation wait for the delay?"""
    import torch
    torch.cuda.synchronize()
    word = torch.zeros(1, device="cuda")
    with torch.cuda.stream(stream):
        enqueue_delay(20.0)
    word.add_(1)
    done = torch.cuda.Event()
    done.record()
    t0 = time.perf_counter()
    while not done.query() and time.perf_counter() - t0 < 0.010:
        pass
    held = not done.query() or stream.query()
    torch.cuda.synchronize()
    return held


def side_stream(k=0):
    """The k-th side stream of the tests: a torch.cuda.Stream() — non-blocking, so the null stream does not wait for it by
    the API's rules — that does not hold the default stream back in practice either.  A device that is given few hardware
    queues puts several streams on one queue, and a stream that shares the default stream's queue would make every control
    clone wait for the delay (late() then fails as vacuous, rightly).  So candidates are probed once, here, and the streams
    found are reused by every test."""
    import torch
    tried = 0
    while len(_side) <= k:
        s = torch.cuda.Stream()
        tried += 1
        assert tried <= 64, "no side stream runs beside the default stream on this device"
        if all(s.cuda_stream != t.cuda_stream for t in _side) and not _holds_back_the_default_stream(s):
            _side.append(s)
    return _side[k]


# ---- answers as bytes: what 'the two references differ' compares ------------------------------------------------------------
def digest(x):
    """a CPU answer — numpy arrays, numbers, tuples / lists / dicts of them, objects that hold them as attributes — as bytes"""
    if x is None:
        return b"N"
    if isinstance(x, np.ndarray):
        return str(x.shape).encode() + np.ascontiguousarray(x).tobytes()
    if isinstance(x, (bool, int, float, str, np.generic)):
        return repr(x).encode()
    if isinstance(x, (tuple, list)):
        return b"(" + b",".join(digest(v) for v in x) + b")"
    if isinstance(x, dict):
        return b"{" + b",".join(str(k).encode() + b":" + digest(v) for k, v in sorted(x.items())) + b"}"
    if hasattr(x, "__dict__"):
        return digest({k: v for k, v in vars(x).items() if isinstance(v, (np.ndarray, bool, int, float, np.generic))})
    raise TypeError(f"digest: {type(x)}")


def answers_differ(a, b):
    return digest(a) != digest(b)


# ---- one case ---------------------------------------------------------------------------------------------------------------
class Report:
    """what late() measured: delay_ms, host_warm_s (the warm-up call's host wall time), host_call_s (the late call's),
    pending (the gate had not fired when the call returned), out (the late call's result)"""


def late(f, real, decoy, stream, check, expect_real, expect_decoy, nonblocking, name="", log=print):
    """One case.  f(X) -> result, called twice under torch.cuda.stream(stream) with X a tuple of device tensors; real, decoy:
    tuples of numpy arrays of equal shapes and dtypes; check(result, expected) raises where a result is not the CPU answer
    `expected` (it may read the result back: the stream is synchronised before it is called); expect_real, expect_decoy: the
    CPU answers.  A case without inputs (real == ()) is judged by its gate and its result alone.  -> Report"""
    import torch
    assert len(real) == len(decoy) and all(r.shape == d.shape and r.dtype == d.dtype for r, d in zip(real, decoy)), name
    if real:
        assert answers_differ(expect_real, expect_decoy), f"{name}: vacuous: the references of the real and the decoy inputs are equal"
    rep = Report()
    with torch.cuda.stream(stream):
        # 1. staging, X = decoy, one synchronous warm-up (fills the allocator's pool of this stream and the mirror's memos)
        real_staged = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in real]
        X = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda().clone() for a in decoy)
        stream.synchronize()
        t0 = time.perf_counter()
        warm = f(X)
        rep.host_warm_s = time.perf_counter() - t0
        stream.synchronize()
        check(warm, expect_decoy)
        for x, d in zip(X, decoy):
            assert x.cpu().numpy().tobytes() == np.ascontiguousarray(d).tobytes(), f"{name}: the call changed its input"
        del warm
        rep.delay_ms = delay_ms_for(rep.host_warm_s)
    # (the control's buffers exist before the delay starts: an allocation that has to go to the device allocator may wait for
    # the device, and the clone would then see the real inputs)
    control = [torch.empty_like(x) for x in X]
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        # 2. the delay, the real inputs behind it, the gate
        enqueue_delay(rep.delay_ms)
        for x, r in zip(X, real_staged):
            x.copy_(r, non_blocking=True)
        gate = torch.cuda.Event()
        gate.record(stream)
    # 3. control, outside the stream: what a launch anywhere else sees
    for c, x in zip(control, X):
        c.copy_(x, non_blocking=True)
    with torch.cuda.stream(stream):
        # 4. the call, 5. the gate
        t0 = time.perf_counter()
        rep.out = f(X)
        rep.host_call_s = time.perf_counter() - t0
        rep.pending = not gate.query()
        # 6. the result
        stream.synchronize()
        log(f"{name}: delay {rep.delay_ms:.0f} ms, warm-up host {1e3 * rep.host_warm_s:.2f} ms, late call host "
            f"{1e3 * rep.host_call_s:.2f} ms, gate {'pending' if rep.pending else 'fired'} on return")
        if nonblocking:
            assert rep.pending, (f"{name}: inconclusive: the gate had fired when the call returned (delay {rep.delay_ms:.0f} ms, "
                                 f"the call took {1e3 * rep.host_call_s:.2f} ms on the host): the call waited, or the delay was too short")
        check(rep.out, expect_real)
        for x, r in zip(X, real):
            assert x.cpu().numpy().tobytes() == np.ascontiguousarray(r).tobytes(), f"{name}: the inputs never arrived"
    torch.cuda.synchronize()
    for c, d in zip(control, decoy):
        assert c.cpu().numpy().tobytes() == np.ascontiguousarray(d).tobytes(), \
            f"{name}: vacuous: the control clone on the default stream did not see the decoy (the delay did not hold the inputs back)"
    return rep

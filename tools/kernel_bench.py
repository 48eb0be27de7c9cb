"""What the kernel benches of this folder share: the timing arguments, the event-timed loop, the alternating race of several routes, the
shader clock and the tail that prints (and optionally writes) the JSON document.  A plain module: a bench imports what it needs."""
import json
import os
import statistics


def add_timing_args(ap, iters, warmup, repeats):
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=iters)
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--repeats", type=int, default=repeats)


def timed(fn, iters, warmup):
    """Microseconds per call: device events around ``iters`` calls after ``warmup`` calls."""
    import torch
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def race(routes, iters, warmup, repeats):
    """``routes``: name -> callable; ``iters``: one count, or name -> count.  -> (medians, all repeats), microseconds per call."""
    times = {name: [] for name in routes}
    for _ in range(repeats):                                        # alternating: drift of the box hits every route alike
        for name, fn in routes.items():
            times[name].append(timed(fn, iters[name] if isinstance(iters, dict) else iters, warmup))
    return {name: statistics.median(v) for name, v in times.items()}, times


def shader_clock():
    from texpose_amd import ops
    return ops.clock_ghz_from_probe(ops.clock_probe())


def finish(res, out_path):
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))

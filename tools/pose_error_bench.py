#!/usr/bin/env python3
"""Time the pose-error kernels (K24 tp_nn1, K25 tp_pose_errors) against the chunked torch route -- texpose_amd/pose_error.py's own
CPU-path code run on the device -- on the same box in the same run, and write profiles/pose_errors/pose_errors.json.

    python tools/pose_error_bench.py [--out profiles/pose_errors/pose_errors.json] [--B 64] [--M 5841 20000 40000]

Per case: a warm-up of both routes, then three alternating repeats, each timed by events on the stream around a call that does no host
synchronisation; the medians are recorded.  Before timing, the two routes' outputs must agree: values by the fp32-grade rule
(e_k <= 2 e_t + 1 ulp against the same torch route in fp64 on the device, on the first --check-poses poses) and, for the search, the
winners' indices equal to the fp64 route's on at least 99 % of the queries (the cap the GPU tests put on near-ties).
Recorded with every search: pair evaluations per second, that figure as fp32 FLOP/s (8 per pair: three subtractions, a product, two
fused multiply-adds) over the 157.3 TFLOP/s vector peak, and as vector instructions (9 per pair) over the issue rate 256 CUs x 64
lanes x the shader clock.  That clock is sampled under load: the probe runs on a side stream while the search of the last (largest)
model runs back to back on the main one for longer than the probe's windows.  A run without a GPU fails: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_FP32_VECTOR = 157.3e12
FLOP_PER_PAIR, VALU_PER_PAIR = 8, 9


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join("profiles", "pose_errors", "pose_errors.json"))
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--M", type=int, nargs="+", default=[5841, 20000, 40000])
    ap.add_argument("--S", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--check-poses", type=int, default=2)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    import torch
    from texpose_amd import ops, pose_error as PE
    if not torch.cuda.is_available():
        raise SystemExit("pose_error_bench: no GPU (nothing is measured without one)")
    dev = torch.device(a.device)
    torch.cuda.set_device(dev)
    rs = np.random.RandomState(0)

    def rotation():
        q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
        q[:, 0] *= np.sign(np.linalg.det(q))
        return q

    def poses(B, base=None):
        out = np.zeros((B, 3, 4), np.float32)
        for b in range(B):
            if base is None:
                out[b, :, :3], out[b, :, 3] = rotation(), rs.uniform(-60, 60, 3) + (0, 0, 1000)
            else:       # a few degrees and millimetres off
                w = rs.normal(size=3) * 0.03
                Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
                out[b, :, :3], out[b, :, 3] = (np.eye(3) + Kx + 0.5 * Kx @ Kx) @ base[b, :, :3], base[b, :, 3] + rs.uniform(-4, 4, 3)
        return out

    def timed(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) * 1e-3

    def compare(name, kernel, torch_route):
        kernel(), torch_route()                                             # warm-up of both
        torch.cuda.synchronize()
        tk, tt = [], []
        for _ in range(a.repeats):                                          # alternating
            tk.append(timed(kernel))
            tt.append(timed(torch_route))
        row = dict(case=name, kernel_s=statistics.median(tk), torch_s=statistics.median(tt), kernel_all_s=tk, torch_all_s=tt)
        row["speedup"] = row["torch_s"] / row["kernel_s"]
        print("%-36s kernel %.6f s   torch route %.6f s   x%.1f" % (name, row["kernel_s"], row["torch_s"], row["speedup"]), flush=True)
        return row

    def rule(name, got, want, t32):
        got, want, t32 = (v.double().cpu().numpy() for v in (got, want, t32))
        e_k, e_t = float(np.abs(got - want).max()), float(np.abs(t32 - want).max())
        floor = float(np.spacing(np.float32(np.abs(want).max())))
        if not e_k <= 2 * e_t + floor:
            raise SystemExit("pose_error_bench: %s disagrees: e_k %.3e, e_t %.3e, floor %.3e" % (name, e_k, e_t, floor))
        return dict(e_k=e_k, e_t=e_t, floor=floor)

    def clock_under_load(load, windows=16, window_us=5000):
        """The shader clock while ``load`` runs: the probe on a side stream, the load back to back on the current one for at least
        twice the probe's windows."""
        load()
        torch.cuda.synchronize()
        calls = max(1, min(1000, int(2.0 * windows * window_us * 1e-6 / max(timed(load), 1e-6)) + 1))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            probe = ops.clock_probe(windows, window_us)
        for _ in range(calls):
            load()
        torch.cuda.synchronize()
        return ops.clock_ghz_from_probe(probe)

    rows = []

    def search_rates(row, pairs):
        row["pairs"] = pairs
        row["pairs_per_s"] = pairs / row["kernel_s"]
        row["fp32_flops_share_of_vector_peak"] = FLOP_PER_PAIR * row["pairs_per_s"] / PEAK_FP32_VECTOR
        return row

    for M in a.M:
        pts = torch.from_numpy(rs.uniform(-100, 100, (M, 3)).astype(np.float32)).to(dev)
        Pg = poses(a.B)
        Pe = torch.from_numpy(poses(a.B, Pg)).to(dev)
        Pg = torch.from_numpy(Pg).to(dev)
        A = PE.relative_pose(Pe, Pg).float()

        def adds_torch(n=a.B, dtype=torch.float32):
            d2, idx = PE.nn1_torch(pts[None].to(dtype), pts[None].to(dtype), A=A[:n].to(dtype))
            return d2.sqrt().mean(-1), idx

        # agreement on the first poses, against the fp64 torch route on the device
        n = min(a.check_poses, a.B)
        want, want_idx = adds_torch(n, torch.float64)
        d2, idx = ops.nn1(pts[None], pts[None], A=A[:n])
        same = float((idx == want_idx).double().mean())
        if same < 0.99:
            raise SystemExit("pose_error_bench: adds M %d: only %.4f of the winners equal the fp64 route's" % (M, same))
        check = rule("adds M %d" % M, d2.sqrt().mean(-1), want, adds_torch(n)[0])
        search_load = lambda pts=pts, A=A: ops.nn1(pts[None], pts[None], A=A)
        # (the kernel side is the public call: it builds A = P_g^-1 P_e itself, a few tiny torch ops, while the torch route is handed
        # the precomputed A -- the kernel side carries that cost, the yardstick does not)
        row = search_rates(compare("adds M %d B %d" % (M, a.B), lambda: PE.adds(pts, Pe, Pg), lambda: adds_torch()), a.B * M * M)
        row.update(check=check, winners_equal=same)
        rows.append(row)

        dia_torch = lambda dtype=torch.float32: PE.nn1_torch(pts[None].to(dtype), pts[None].to(dtype), mode="farthest")[0].max().sqrt()
        check = rule("model_diameter M %d" % M, PE.model_diameter(pts), dia_torch(torch.float64), dia_torch())
        row = search_rates(compare("model_diameter M %d" % M, lambda: PE.model_diameter(pts), dia_torch), M * M)
        row.update(check=check)
        rows.append(row)

        K = torch.tensor([[572.4, 0, 325.3], [0, 573.6, 242.0], [0, 0, 1]], device=dev).repeat(a.B, 1, 1)
        for S in a.S:
            sym = np.stack([np.eye(3, 4)] + [np.concatenate([rotation(), rs.uniform(-3, 3, (3, 1))], 1) for _ in range(S - 1)])
            sym = torch.from_numpy(sym.astype(np.float32)).to(dev)
            got = ops.pose_errors(pts, Pe, Pg, sym, K)
            t32 = PE.pose_errors_torch(pts, Pe, Pg, sym, K)
            t64 = PE.pose_errors_torch(pts.double(), Pe, Pg, sym, K)
            check = {k: rule("%s M %d S %d" % (k, M, S), got[k], t64[k], t32[k]) for k in ("add", "mssd", "mspd", "proj")}
            for k in ("s_mssd", "s_mspd"):
                if not torch.equal(got[k], t64[k]):
                    raise SystemExit("pose_error_bench: %s M %d S %d differs from the fp64 route" % (k, M, S))
            row = compare("pose_errors M %d B %d S %d" % (M, a.B, S), lambda: ops.pose_errors(pts, Pe, Pg, sym, K),
                          lambda: PE.pose_errors_torch(pts, Pe, Pg, sym, K))
            row.update(check=check)
            rows.append(row)

    clock = clock_under_load(search_load)
    issue_rate = 256 * 64 * clock * 1e9
    for row in rows:
        if "pairs_per_s" in row:
            row["valu_issue_share"] = VALU_PER_PAIR * row["pairs_per_s"] / issue_rate
    result = dict(device=torch.cuda.get_device_name(dev), shader_clock_ghz=clock, repeats=a.repeats, B=a.B,
                  peak_fp32_vector_flops=PEAK_FP32_VECTOR, valu_issue_rate_lane_ops=issue_rate, cases=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("pose_error_bench: %d cases at %.3f GHz -> %s" % (len(rows), clock, a.out))


if __name__ == "__main__":
    main()

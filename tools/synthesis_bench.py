"""Novel-view synthesis with the inference-only f16 MLP arithmetic: speed and image fidelity against f16x3.

Times full-image Graph.render_by_slices(mode="eval_noalign") at 480x640 for each --samples value, the f16x3 and f16 arms
alternated in one process (--images timed images per arm after one warm-up image), and compares each arm's image with the
exact-fp32 kernel's: max / rms abs error of rgb_static, depth rel-L2, opacity max abs, the 8-bit image (mul(255).byte(), as the
reference's to_pil_image writes it) and PSNR / SSIM of the project's evaluation metrics against a target image (the exact
render plus fixed noise: the synthetic scene has no photograph).  Prints one JSON document.

    python tools/synthesis_bench.py [--samples 128 64] [--images 3] [--checkpoint PATH]

--checkpoint: a reference-format checkpoint (texpose_amd.checkpoint) whose network replaces the synthetic weights, so that
users can check the fidelity of their own pretrained trunk.  Kernel time: run the script under
rocprofv3 --kernel-trace --stats -- python tools/synthesis_bench.py ...
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from texpose_amd import ops  # noqa: E402

H, W = bench.H, bench.W


def load_network(path, graph):
    """the nerf.mlp_* tensors of a reference-format checkpoint ({"graph": state dict}) into the render network"""
    ckpt = torch.load(path, map_location="cpu")
    state = ckpt.get("graph", ckpt)
    nerf = {k[len("nerf."):]: v for k, v in state.items() if k.startswith("nerf.mlp_")}
    if not nerf:
        raise SystemExit("--checkpoint: no nerf.mlp_* tensors in %s" % path)
    dev = next(graph.nerf.parameters()).device
    graph.nerf.load_state_dict({**graph.nerf.state_dict(), **{k: v.to(dev) for k, v in nerf.items()}})
    return len(nerf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, nargs="+", default=[128, 64])
    ap.add_argument("--images", type=int, default=3)
    ap.add_argument("--checkpoint", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sc, params, emb_t, emb_l = bench.build_scene(dev, 0)
    graph, opt = bench.make_graph(dev, params, emb_t, emb_l)
    if args.checkpoint:
        load_network(args.checkpoint, graph)
    opt.nerf.sample_stratified = False
    pose, intr = sc["pose"].to(dev), sc["intr"].to(dev)
    dr = (sc["z_near"].to(dev)[:, :, None], sc["z_far"].to(dev)[:, :, None])
    mask = torch.ones(1, H, W, device=dev)
    sidx = torch.tensor(0, device=dev)

    def render(prec):
        graph.nerf.precision = prec
        with torch.no_grad():
            return graph.render_by_slices(opt, pose, intr=intr, depth_range=dr, object_mask=mask, sample_idx=sidx, mode="eval_noalign")

    result = {"H": H, "W": W, "checkpoint": args.checkpoint, "images_per_arm": args.images, "configs": []}
    for n in args.samples:
        opt.nerf.sample_intvs = n
        exact = render("fp32")
        gen = torch.Generator().manual_seed(5)
        noise = torch.randn(1, 3, H, W, generator=gen).to(dev) * 0.02
        target = (exact["rgb_static"].view(1, H, W, 3).permute(0, 3, 1, 2) + noise).clamp(0, 1).contiguous()
        outs, times = {}, {"f16x3": [], "f16": []}
        for prec in ("f16x3", "f16"):
            outs[prec] = render(prec)                      # warm-up (packs the stream)
        for _ in range(args.images):
            for prec in ("f16x3", "f16"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs[prec] = render(prec)
                torch.cuda.synchronize()
                times[prec].append(time.perf_counter() - t0)
        ops.check_mlp_status(dev)
        cfg = {"N": n, "ray_bias_form": ops.ray_bias_applies("f16", n, False, True), "arms": {}}
        e8 = (exact["rgb_static"].clamp(0, 1) * 255).byte()
        ps_e, ss_e, _ = ops.eval_metrics(exact["rgb_static"].view(1, H * W, 3), target, mask, H, W)
        for prec in ("f16x3", "f16"):
            o = outs[prec]
            ms = 1e3 * float(np.median(times[prec]))
            d = (o["rgb_static"] - exact["rgb_static"]).double()
            o8 = (o["rgb_static"].clamp(0, 1) * 255).byte()
            d8 = (o8.int() - e8.int()).abs()
            dep = o["depth"].double()
            ps, ss, _ = ops.eval_metrics(o["rgb_static"].view(1, H * W, 3), target, mask, H, W)
            cfg["arms"][prec] = {
                "ms_per_image": ms, "ms_all": [1e3 * t for t in times[prec]], "rays_per_s": H * W / (ms / 1e3),
                "rgb_static_max_abs": float(d.abs().max()), "rgb_static_rms": float(d.pow(2).mean().sqrt()),
                "depth_rel_l2": float((dep - exact["depth"].double()).norm() / exact["depth"].double().norm()),
                "opacity_max_abs": float((o["opacity"] - exact["opacity"]).abs().max()),
                "u8_max_diff": int(d8.max()), "u8_share_differing": float((d8 > 0).double().mean()),
                "psnr": float(ps), "ssim": float(ss), "psnr_minus_exact": float(ps - ps_e), "ssim_minus_exact": float(ss - ss_e)}
        cfg["exact_psnr"], cfg["exact_ssim"] = float(ps_e), float(ss_e)
        cfg["rays_per_s_ratio_f16_over_f16x3"] = cfg["arms"]["f16"]["rays_per_s"] / cfg["arms"]["f16x3"]["rays_per_s"]
        result["configs"].append(cfg)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()

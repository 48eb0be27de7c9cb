#!/usr/bin/env python3
"""Write the surfel maps of one adaptation loop (rgbsyn_<loop>/, nocs_<loop>/, normal_<loop>/) for a CAD mesh at predicted poses,
in place of the reference's compute_surfelinfo.py (its PyTorch3D renderer does not exist on ROCm).

    python tools/surfel_maps.py --ply models/obj_000009.ply --poses pred.npz --depth-scale 10 --loop 0 --out <sequence dir>

--poses: an .npz with frame_index [N], pose [N,3,4] (t in nerf.depth.scale units, like pose_init) and intr [N,3,3] or [3,3].
--out is the directory data/lm.py reads the maps from (data_path/<folder>).  --obj-scene-id writes the multi-object names.
--verify-online: after writing, read the files back as the data layer does (8-bit decode, alpha > 0, smooth_geo) and compare them with
SurfelRenderer.data_layer_maps, the in-process route that needs no files; the exit status is non-zero if any tensor differs."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ply", required=True)
    ap.add_argument("--poses", required=True)
    ap.add_argument("--depth-scale", type=float, required=True, help="nerf.depth.scale of the run (pose t * 1000 / scale = mm)")
    ap.add_argument("--H", type=int, default=480)
    ap.add_argument("--W", type=int, default=640)
    ap.add_argument("--loop", required=True, help="pose_loop: the files go to rgbsyn_<loop>/ nocs_<loop>/ normal_<loop>/")
    ap.add_argument("--out", required=True)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--obj-scene-id", type=int, default=None)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--verify-online", action="store_true", help="decode the written files and compare with data_layer_maps")
    a = ap.parse_args(argv)
    import torch
    from texpose_amd.surfel import MAP_KEYS, SurfelRenderer, load_ply, read_surfel_frame, write_surfel_frame
    verts, faces, vcolor = load_ply(a.ply)
    z = np.load(a.poses)
    frames, pose, intr = z["frame_index"].astype(np.int64).reshape(-1), z["pose"].astype(np.float32), z["intr"].astype(np.float32)
    if intr.ndim == 2:
        intr = np.broadcast_to(intr, (len(frames), 3, 3))
    if pose.shape != (len(frames), 3, 4) or intr.shape != (len(frames), 3, 3):
        raise SystemExit("--poses: frame_index [N], pose [N,3,4], intr [N,3,3] or [3,3] expected")
    renderer = SurfelRenderer(verts, faces, vcolor, a.H, a.W, a.device)
    t0 = time.time()
    for s in range(0, len(frames), a.batch):
        out = renderer(torch.from_numpy(pose[s:s + a.batch]), torch.from_numpy(np.ascontiguousarray(intr[s:s + a.batch])), a.depth_scale)
        for b in range(out.depth.shape[0]):
            write_surfel_frame(a.out, a.loop, int(frames[s + b]), out, b, a.obj_scene_id)
    print("surfel_maps: %d frames, %d faces, %dx%d -> %s (%.2f s)" % (len(frames), len(faces), a.H, a.W, a.out, time.time() - t0))
    if a.verify_online:
        bad = 0
        for s in range(0, len(frames), a.batch):
            maps = renderer.data_layer_maps(torch.from_numpy(pose[s:s + a.batch]), torch.from_numpy(np.ascontiguousarray(intr[s:s + a.batch])),
                                            a.depth_scale)
            for b in range(maps.depth.shape[0]):
                dec = read_surfel_frame(a.out, a.loop, int(frames[s + b]), a.obj_scene_id)
                for k in MAP_KEYS:
                    if not torch.equal(maps[k][b].cpu(), dec[k]):
                        bad += 1
                        print("surfel_maps: frame %d: %s differs from the decoded files in %d values"
                              % (int(frames[s + b]), k, int((maps[k][b].cpu() != dec[k]).sum())))
        print("surfel_maps: verify-online: %d frames x %d tensors, %s" % (len(frames), len(MAP_KEYS), "all equal" if not bad else "%d DIFFER" % bad))
        if bad:
            raise SystemExit(1)


if __name__ == "__main__":
    main()

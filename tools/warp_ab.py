"""A/B of the affine warp on the GPU (backend.Warp and
GpuDecoder.decode_rgb_warped()) against what it generalises and what it
replaces, one device, same run.

    python tools/warp_ab.py [--frames 256] [--rounds 10] [--out profiles/warp_ab.json]

First, on a small case (three sources of different sizes, both border modes),
Warp's output must equal the numpy model's (tests/warp_model.py) bit for bit in
both ways of dealing the output to the waves.

(a) The kernel alone.  `frames` planar uint8 FHD frames (3 x 1080 x 1920 random
bytes each) to 224 x 224 float16 with ImageNet constants, one launch:
  resize          backend.Resize on the same data: the baseline
  warp_axis       Warp with the axis-aligned matrix of that resize (the same
                  taps up to the weights' definition): the price of generality
  rot30_rowmajor  a 30 degree turn at the same zoom (1080 / 224), a wave taking
  rot30_tiled     64 consecutive quads of a row / a tile of 8 quads x 8 rows
  rot30z15_*      the same turn at zoom 1.5: the dense taps of a warp behind a
                  scaled or ROI decode
  copy            a device copy of the bytes written (Tensor.copy_)
Device events around `--reps` back-to-back launches; the legs alternate inside
every round; medians with min and max.

(b) End to end.  `frames` q90 4:2:0 FHD JPEGs (bench.py's synthetic files, a
pool of distinct ones cycled), each with its own angle in +-30 degrees and
zoom in 1..2, to 224 x 224 float16 with ImageNet mean / std:
  warped   decode_rgb_warped(size, xforms, dtype=float16, mean=, std=)
  torch    the route it replaces: decode_rgb() to uint8 planes, then per image
           affine_grid + grid_sample (float32, zeros padding) and the
           normalisation, rounded to half
Host clock around the call with a device synchronise before and inside the
window; interleaved rounds after untimed warm rounds.  Before timing, the two
must agree per channel within (0.5 + 2 * 255 / 2048 + 0.1) * a[c] + 2^-9 in
normalised units: the definition's bound against real bilinear (include/hjd.h),
0.1 grey level for the float32 grid and blend of the torch route, scaled by
the channel's a = 1 / (255 std), plus the two roundings to half.  The torch
route is given the integer matrices' own values (m / 65536), so the matrices'
quantisation is not in the comparison.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
W, H = 1920, 1080
OUT = 224
POOL = 8
BOUND = 0.5 + 2 * 255 / 2048


def stats(v):
    return {"ms_min": round(min(v), 4), "ms_median": round(statistics.median(v), 4), "ms_max": round(max(v), 4),
            "ms_rounds": [round(t, 4) for t in v]}


def model_check(torch, hjd, ctx, dev):
    """Warp against tests/warp_model.py on a small case, both forms, bit for bit."""
    import warp_model
    shapes = [(37, 29), (80, 40), (5, 3)]
    wo, ho = 24, 16
    xf = [hjd.warp_xform(37, 29, wo, ho, angle=30.0, zoom=1.3), hjd.warp_xform(80, 40, wo, ho, zoom=0.5, center=(78.0, 1.5)),
          [65536, 3000, 9 << 16, -2000, 65536, 1 << 16]]
    fills, repl = [0x102030, 0, 0xC0FFEE], [False, True, False]
    a, b = hjd.norm_constants(MEAN, STD)
    rng = np.random.default_rng(7)
    host = [rng.integers(0, 256, (3, h, w), dtype=np.uint8) for w, h in shapes]
    srcs = [torch.from_numpy(s).to(dev) for s in host]
    out = torch.zeros((3, 3, ho, wo), dtype=torch.float16, device=dev)
    op = hjd.Warp(ctx, srcs, out, xf, fills=fills, replicate=repl, normalize=(a, b))
    for form in (None, False, True):
        out.zero_()
        if form is None:
            op.launch(torch.cuda.current_stream())
        else:
            op.launch_form(form, torch.cuda.current_stream())
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint16)
        for k in range(3):
            exp = warp_model.warp(host[k], xf[k], wo, ho, fills[k], 1 if repl[k] else 0, np.float16,
                                  tuple(float(v) for v in a), tuple(float(v) for v in b))
            if not np.array_equal(got[k], exp):
                raise SystemExit(f"item {k}, form {form}: Warp differs from the model")
    op.close()


def axis_matrix(src_w, src_h, out_w, out_h):
    """The resize's map as a warp: X = (j + 0.5) src_w / out_w - 0.5, in Q16."""
    sx, sy = src_w / out_w, src_h / out_h
    return [round(sx * 65536), 0, round((sx / 2 - 0.5) * 65536), 0, round(sy * 65536), round((sy / 2 - 0.5) * 65536)]


def kernel_alone(torch, hjd, ctx, dev, nf, rounds, warm_rounds, reps):
    gen = torch.Generator(device=dev).manual_seed(5)
    src = torch.randint(0, 256, (nf, 3, H, W), dtype=torch.uint8, device=dev, generator=gen)
    srcs = [src[i] for i in range(nf)]
    norm = hjd.norm_constants(MEAN, STD)
    stream = torch.cuda.current_stream()
    outs = {name: torch.zeros((nf, 3, OUT, OUT), dtype=torch.float16, device=dev)
            for name in ("resize", "warp_axis", "rot30", "rot30z15")}
    copy_dst = torch.empty_like(outs["resize"])
    resize = hjd.Resize(ctx, srcs, outs["resize"], normalize=norm)
    axis = hjd.Warp(ctx, srcs, outs["warp_axis"], [axis_matrix(W, H, OUT, OUT)] * nf, replicate=True, normalize=norm)
    rot = hjd.Warp(ctx, srcs, outs["rot30"], [hjd.warp_xform(W, H, OUT, OUT, angle=30.0, zoom=H / OUT)] * nf,
                   normalize=norm)
    rot15 = hjd.Warp(ctx, srcs, outs["rot30z15"], [hjd.warp_xform(W, H, OUT, OUT, angle=30.0, zoom=1.5)] * nf,
                     normalize=norm)
    legs = {"copy": lambda: copy_dst.copy_(outs["resize"]),
            "resize": lambda: resize.launch(stream),
            "warp_axis": lambda: axis.launch(stream),
            "rot30_rowmajor": lambda: rot.launch_form(False, stream),
            "rot30_tiled": lambda: rot.launch_form(True, stream),
            "rot30z15_rowmajor": lambda: rot15.launch_form(False, stream),
            "rot30z15_tiled": lambda: rot15.launch_form(True, stream)}
    # the axis-aligned warp computes the resize's picture: the two definitions place their weights
    # within 1 / 2048 pixel of each other, so the bytes agree within one grey level (here: of the half values)
    resize.launch(stream)
    axis.launch(stream)
    torch.cuda.synchronize()
    a_max = float(max(norm[0]))
    axis_diff = float((outs["resize"].float() - outs["warp_axis"].float()).abs().max())
    if axis_diff > 2.0 * a_max + 2.0 ** -9:
        raise SystemExit(f"the axis-aligned warp differs from the resize by {axis_diff} in normalised units")
    # and the two forms of one launch write the same bytes
    rot.launch_form(False, stream)
    torch.cuda.synchronize()
    first = outs["rot30"].clone()
    rot.launch_form(True, stream)
    torch.cuda.synchronize()
    if not torch.equal(first.view(torch.int16), outs["rot30"].view(torch.int16)):
        raise SystemExit("the row-major and the tiled launch differ")
    del first

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    for _ in range(max(1, warm_rounds)):
        for fn in legs.values():
            timed(fn)
    ms = {name: [] for name in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            ms[name].append(timed(fn))
    res = {"frames": nf, "width": W, "height": H, "out": [OUT, OUT], "dtype": "float16", "launches_per_sample": reps,
           "bytes_written": outs["resize"].numel() * 2, "max_abs_diff_warp_axis_vs_resize": axis_diff,
           "timing": "device events around the back-to-back launches, per launch",
           "legs": {name: stats(v) for name, v in ms.items()}}
    L = res["legs"]
    copy_med = L["copy"]["ms_median"]
    for leg in L.values():
        leg["vs_copy"] = round(leg["ms_median"] / copy_med, 4)
    res["holds"] = {"warp_axis_vs_resize": round(L["warp_axis"]["ms_median"] / L["resize"]["ms_median"], 4),
                    "rot30_tiled_vs_rowmajor": round(L["rot30_tiled"]["ms_median"] / L["rot30_rowmajor"]["ms_median"], 4),
                    "rot30z15_tiled_vs_rowmajor": round(L["rot30z15_tiled"]["ms_median"] /
                                                        L["rot30z15_rowmajor"]["ms_median"], 4)}
    for op in (resize, axis, rot, rot15):
        op.close()
    del src, srcs, outs, copy_dst
    torch.cuda.empty_cache()
    return res


def theta_of(m, src_w, src_h, out_w, out_h):
    """affine_grid's theta (align_corners=False) of the integer matrix m."""
    M = [v / 65536.0 for v in m]
    rows = []
    for (mj, mi, t), size in ((M[0:3], src_w), (M[3:6], src_h)):
        rows.append([mj * out_w / size, mi * out_h / size,
                     (2.0 / size) * (mj * (out_w - 1) / 2 + mi * (out_h - 1) / 2 + t + 0.5) - 1.0])
    return rows


def end_to_end(torch, hjd, ctx, dev, nf, rounds, warm_rounds):
    import bench
    pool = bench.encode_pool(W, H, hjd.YUV420, min(POOL, nf), seed0=9400)
    datas = [pool[i % len(pool)] for i in range(nf)]
    rng = np.random.default_rng(11)
    angles, zooms = rng.uniform(-30.0, 30.0, nf), rng.uniform(1.0, 2.0, nf)
    xf = [hjd.warp_xform(W, H, OUT, OUT, angle=float(a), zoom=float(z)) for a, z in zip(angles, zooms)]
    thetas = torch.tensor([theta_of(m, W, H, OUT, OUT) for m in xf], dtype=torch.float32, device=dev)
    info = hjd.parse(datas[0])
    a_np, b_np = hjd.norm_constants(MEAN, STD)
    a32 = torch.tensor(a_np, device=dev).view(1, 3, 1, 1)
    b32 = torch.tensor(b_np, device=dev).view(1, 3, 1, 1)
    gd = hjd.GpuDecoder(ctx, nf, 2 * sum(map(len, datas)), nf * info.nblocks)
    F = torch.nn.functional
    last = {}

    def leg_warped():
        last["warped"] = gd.decode_rgb_warped(datas, (OUT, OUT), xf, dtype=torch.float16, mean=MEAN, std=STD)
        gd.sync()

    def leg_torch():
        planes = gd.decode_rgb(datas)
        gd.sync()
        out = torch.empty((nf, 3, OUT, OUT), dtype=torch.float16, device=dev)
        for i, p in enumerate(planes):
            grid = F.affine_grid(thetas[i:i + 1], (1, 3, OUT, OUT), align_corners=False)
            s = F.grid_sample(p[None].float(), grid, mode="bilinear", padding_mode="zeros", align_corners=False)
            out[i] = torch.addcmul(b32, s, a32)[0].half()
        last["torch"] = out

    jobs = [("warped", leg_warped), ("torch", leg_torch)]
    for _ in range(max(1, warm_rounds)):
        for _, job in jobs:
            job()
    torch.cuda.synchronize()
    diff = (last["warped"].float() - last["torch"].float()).abs().amax(dim=(0, 2, 3)).cpu().tolist()
    tol = [(BOUND + 0.1) * float(a) + 2.0 ** -9 for a in a_np]
    if any(d > t for d, t in zip(diff, tol)):
        raise SystemExit(f"the warped decode and the torch route differ by {diff} per channel (tolerance {tol})")
    rois = [hjd.warp_roi(W, H, m, OUT, OUT) for m in xf]

    def timed_wall(job):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        job()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    ms = {name: [] for name, _ in jobs}
    for _ in range(rounds):
        for name, job in jobs:
            ms[name].append(timed_wall(job))
    res = {"frames": nf, "width": W, "height": H, "out": [OUT, OUT], "distinct_files": len(pool),
           "jpeg_bytes": sum(map(len, datas)), "dtype": "float16", "angle_degrees": [-30, 30], "zoom": [1, 2],
           "decoded_pixel_fraction": round(sum(r[2] * r[3] for r in rois) / (nf * W * H), 4),
           "max_abs_diff_torch_vs_warped_per_channel": diff, "tolerance_per_channel": tol,
           "timing": "host clock around the call, a device synchronise before and inside the window",
           "legs": {name: stats(v) for name, v in ms.items()}}
    L = res["legs"]
    res["holds"] = {"warped_vs_torch": round(L["warped"]["ms_median"] / L["torch"]["ms_median"], 4),
                    "warped_below_torch": L["warped"]["ms_median"] < L["torch"]["ms_median"]}
    gd.close()
    last.clear()
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warm-rounds", type=int, default=2, help="untimed interleaved rounds before the timed ones")
    ap.add_argument("--reps", type=int, default=20, help="(a): back-to-back launches per timed sample")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "warp_ab.json"))
    args = ap.parse_args()
    import torch
    import ocljpegdecoder_amd as hjd
    if not torch.cuda.is_available():
        raise SystemExit("warp_ab needs a GPU: no timing is taken without one")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = hjd.Context(0)
    result = {"tool": "tools/warp_ab.py", "utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
              "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "frames": args.frames,
              "rounds": args.rounds, "warm_rounds": args.warm_rounds, "mean": list(MEAN), "std": list(STD),
              "method": "untimed interleaved warm rounds of every leg, then interleaved rounds; medians with min and max"}
    model_check(torch, hjd, ctx, dev)
    result["model_check"] = "Warp == tests/warp_model.py on 3 items, 24 x 16 float16, both forms"
    result["kernel_alone"] = kernel_alone(torch, hjd, ctx, dev, args.frames, args.rounds, args.warm_rounds, args.reps)
    for name, leg in result["kernel_alone"]["legs"].items():
        print(f"kernel {name:18s} {leg['ms_median']:9.4f} ms (median) {leg['ms_min']:9.4f} (min) {leg['ms_max']:9.4f} (max) "
              f"x{leg['vs_copy']} of the copy", file=sys.stderr, flush=True)
    print("holds", json.dumps(result["kernel_alone"]["holds"]), file=sys.stderr, flush=True)
    result["end_to_end"] = end_to_end(torch, hjd, ctx, dev, args.frames, args.rounds, args.warm_rounds)
    for name, leg in result["end_to_end"]["legs"].items():
        print(f"e2e {name:10s} {leg['ms_median']:9.3f} ms (median) {leg['ms_min']:9.3f} (min) {leg['ms_max']:9.3f} (max)",
              file=sys.stderr, flush=True)
    print("holds", json.dumps(result["end_to_end"]["holds"]), file=sys.stderr, flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"warp_ab": "ok", "file": os.path.relpath(args.out, REPO)}))


if __name__ == "__main__":
    main()

"""A/B of the colour stage on the GPU (backend.Color and
GpuDecoder.decode_rgb_resized_color()) against the route it replaces, one
device, same run.

    python tools/color_ab.py [--frames 256] [--rounds 10] [--out profiles/color_ab.json]
    python tools/color_ab.py --resized-only     # only decode_rgb_resized on workload (b): for a parent / branch A/B

First, on a small case (three sources of different sizes, one record with a
p), Color's output must equal the numpy model's (tests/color_model.py) bit for
bit.

(a) The kernels alone.  `frames` x 3 x 224 x 224 random bytes to float16 with
ImageNet constants:
  color_m   Color with records whose p is 0: one launch
  color_p   Color with records that read the means: the summing launch and the
            colour launch
  copy_u8   a device copy of the bytes read (Tensor.copy_)
  copy_f16  a device copy of the bytes written
Device events around `--reps` back-to-back launches; the legs alternate inside
every round; medians with min and max.

(b) End to end.  `frames` q90 4:2:0 FHD JPEGs (bench.py's synthetic files, a
pool of distinct ones cycled), each with its own random-resized crop (8 % ..
100 % of the area, aspect 3/4 .. 4/3), flip and jitter (brightness, contrast,
saturation in 0.6 .. 1.4, hue in +-0.1 turns), to 224 x 224 float16 with
ImageNet mean / std:
  color    decode_rgb_resized_color(size, rois=, flips=, colors=, dtype=float16, mean=, std=)
  resized  decode_rgb_resized(...) of the same crops to float16 without colours: what the stage adds to
  torch    the route it replaces: decode_rgb_resized() to uint8, then in torch
           the per-image channel means, einsum with the real matrices, clamp,
           round and the normalisation, rounded to half
Host clock around the call with a device synchronise before and inside the
window; interleaved rounds after untimed warm rounds.  Before timing, `color`
and `torch` must agree within one grey level: 1 * a[c] + 2^-9 in normalised
units.  The integer stage is within 0.5 + 2^-13 + 24 * 2^-9 < 0.55 of the real
map of its own record (include/hjd.h), the torch route is given that record's
values (m / 4096) and rounds its float32 result itself, so where the real
value lies near a half the two bytes differ by one; the two roundings to half
add 2^-9.
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


def stats(v):
    return {"ms_min": round(min(v), 4), "ms_median": round(statistics.median(v), 4), "ms_max": round(max(v), 4),
            "ms_rounds": [round(t, 4) for t in v]}


def model_check(torch, hjd, ctx, dev):
    """Color against tests/color_model.py on a small case, bit for bit."""
    import color_model
    shapes = [(37, 29), (64, 4), (5, 3)]
    recs = [hjd.color_matrix(brightness=1.2, contrast=0.6, saturation=1.4, hue=0.1), hjd.color_matrix(invert=True),
            hjd.color_matrix(contrast=1.5, pivot=100, gray=True)]
    a, b = hjd.norm_constants(MEAN, STD)
    rng = np.random.default_rng(7)
    host = [rng.integers(0, 256, (3, h, w), dtype=np.uint8) for w, h in shapes]
    srcs = [torch.from_numpy(s).to(dev) for s in host]
    outs = [torch.zeros(s.shape, dtype=torch.float16, device=dev) for s in host]
    op = hjd.Color(ctx, srcs, outs, recs, normalize=(a, b))
    op.launch(torch.cuda.current_stream())
    torch.cuda.synchronize()
    op.close()
    for k in range(3):
        exp = color_model.color(host[k], recs[k], np.float16, tuple(float(v) for v in a), tuple(float(v) for v in b))
        if not np.array_equal(outs[k].cpu().numpy().view(np.uint16), exp):
            raise SystemExit(f"item {k}: Color differs from the model")


def jitter(hjd, rng, n):
    """n records of a ColorJitter(0.4, 0.4, 0.4, 0.1) draw, with contrast about the mean."""
    recs = []
    for _ in range(n):
        b, c, s = (float(v) for v in rng.uniform(0.6, 1.4, 3))
        recs.append(hjd.color_matrix(brightness=b, contrast=c, saturation=s, hue=float(rng.uniform(-0.1, 0.1))))
    return recs


def kernel_alone(torch, hjd, ctx, dev, nf, rounds, warm_rounds, reps):
    gen = torch.Generator(device=dev).manual_seed(5)
    src = torch.randint(0, 256, (nf, 3, OUT, OUT), dtype=torch.uint8, device=dev, generator=gen)
    srcs = [src[i] for i in range(nf)]
    norm = hjd.norm_constants(MEAN, STD)
    stream = torch.cuda.current_stream()
    rng = np.random.default_rng(3)
    with_p = jitter(hjd, rng, nf)
    no_p = [r[:9] + [0] * 9 + r[18:] for r in with_p]
    out_m = torch.zeros((nf, 3, OUT, OUT), dtype=torch.float16, device=dev)
    out_p = torch.zeros_like(out_m)
    copy_u8, copy_f16 = torch.empty_like(src), torch.empty_like(out_m)
    color_m = hjd.Color(ctx, srcs, out_m, no_p, normalize=norm)
    color_p = hjd.Color(ctx, srcs, out_p, with_p, normalize=norm)
    legs = {"copy_u8": lambda: copy_u8.copy_(src),
            "copy_f16": lambda: copy_f16.copy_(out_m),
            "color_m": lambda: color_m.launch(stream),
            "color_p": lambda: color_p.launch(stream)}

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
    res = {"frames": nf, "size": [OUT, OUT], "dtype": "float16", "launches_per_sample": reps,
           "bytes_read": src.numel(), "bytes_written": out_m.numel() * 2,
           "timing": "device events around the back-to-back launches, per launch",
           "legs": {name: stats(v) for name, v in ms.items()}}
    L = res["legs"]
    for leg in L.values():
        leg["vs_copy_f16"] = round(leg["ms_median"] / L["copy_f16"]["ms_median"], 4)
    res["holds"] = {"color_p_vs_color_m": round(L["color_p"]["ms_median"] / L["color_m"]["ms_median"], 4)}
    for op in (color_m, color_p):
        op.close()
    del src, srcs, out_m, out_p, copy_u8, copy_f16
    torch.cuda.empty_cache()
    return res


def crops(rng, n):
    """RandomResizedCrop's rectangles on a W x H frame: (x, y, w, h) per image."""
    rois = []
    for _ in range(n):
        area = rng.uniform(0.08, 1.0) * W * H
        ratio = np.exp(rng.uniform(np.log(3 / 4), np.log(4 / 3)))
        w = int(min(W, max(1, round(np.sqrt(area * ratio)))))
        h = int(min(H, max(1, round(np.sqrt(area / ratio)))))
        rois.append((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
    return rois


def end_to_end(torch, hjd, ctx, dev, nf, rounds, warm_rounds, resized_only):
    import bench
    pool = bench.encode_pool(W, H, hjd.YUV420, min(POOL, nf), seed0=9400)
    datas = [pool[i % len(pool)] for i in range(nf)]
    rng = np.random.default_rng(11)
    rois = crops(rng, nf)
    flips = [bool(v) for v in rng.integers(0, 2, nf)]
    info = hjd.parse(datas[0])
    gd = hjd.GpuDecoder(ctx, nf, 2 * sum(map(len, datas)), nf * info.nblocks)
    last = {}

    def leg_resized():
        last["resized"] = gd.decode_rgb_resized(datas, (OUT, OUT), flips=flips, rois=rois, dtype=torch.float16,
                                                mean=MEAN, std=STD)
        gd.sync()

    jobs = [("resized", leg_resized)]
    if not resized_only:
        recs = jitter(hjd, rng, nf)
        q = torch.tensor(recs, dtype=torch.float32, device=dev) / 4096.0
        Mr, Pr, tr = q[:, :9].view(nf, 3, 3), q[:, 9:18].view(nf, 3, 3), q[:, 18:]
        a_np, b_np = hjd.norm_constants(MEAN, STD)
        a32 = torch.tensor(a_np, device=dev).view(1, 3, 1, 1)
        b32 = torch.tensor(b_np, device=dev).view(1, 3, 1, 1)

        def leg_color():
            last["color"] = gd.decode_rgb_resized_color(datas, (OUT, OUT), flips=flips, rois=rois, colors=recs,
                                                        dtype=torch.float16, mean=MEAN, std=STD)
            gd.sync()

        def leg_torch():
            u8 = gd.decode_rgb_resized(datas, (OUT, OUT), flips=flips, rois=rois)
            gd.sync()
            x = u8.float()
            off = torch.einsum("ncd,nd->nc", Pr, x.mean(dim=(2, 3))) + tr
            y = torch.einsum("ncd,ndhw->nchw", Mr, x) + off[:, :, None, None]
            last["torch"] = torch.addcmul(b32, y.clamp_(0.0, 255.0).round_(), a32).half()

        jobs += [("color", leg_color), ("torch", leg_torch)]
    for _ in range(max(1, warm_rounds)):
        for _, job in jobs:
            job()
    torch.cuda.synchronize()
    res = {"frames": nf, "width": W, "height": H, "out": [OUT, OUT], "distinct_files": len(pool),
           "jpeg_bytes": sum(map(len, datas)), "dtype": "float16", "crop_area": [0.08, 1.0],
           "decoded_pixel_fraction": round(sum(r[2] * r[3] for r in rois) / (nf * W * H), 4),
           "timing": "host clock around the call, a device synchronise before and inside the window"}
    if not resized_only:
        diff = (last["color"].float() - last["torch"].float()).abs().amax(dim=(0, 2, 3)).cpu().tolist()
        tol = [float(a) + 2.0 ** -9 for a in a_np]
        if any(d > t for d, t in zip(diff, tol)):
            raise SystemExit(f"the colour decode and the torch route differ by {diff} per channel (tolerance {tol})")
        res.update({"jitter": "brightness, contrast, saturation in 0.6..1.4, hue in +-0.1 turns, contrast about the mean",
                    "max_abs_diff_torch_vs_color_per_channel": diff, "tolerance_per_channel": tol})

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
    res["legs"] = L = {name: stats(v) for name, v in ms.items()}
    if not resized_only:
        res["holds"] = {"color_vs_torch": round(L["color"]["ms_median"] / L["torch"]["ms_median"], 4),
                        "color_minus_resized_ms": round(L["color"]["ms_median"] - L["resized"]["ms_median"], 4),
                        "color_below_torch": L["color"]["ms_median"] < L["torch"]["ms_median"]}
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
    ap.add_argument("--resized-only", action="store_true",
                    help="time only decode_rgb_resized on workload (b): runs on a library without the colour stage")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "color_ab.json"))
    args = ap.parse_args()
    import torch
    import ocljpegdecoder_amd as hjd
    if not torch.cuda.is_available():
        raise SystemExit("color_ab needs a GPU: no timing is taken without one")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = hjd.Context(0)
    result = {"tool": "tools/color_ab.py", "utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
              "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "frames": args.frames,
              "rounds": args.rounds, "warm_rounds": args.warm_rounds, "mean": list(MEAN), "std": list(STD),
              "method": "untimed interleaved warm rounds of every leg, then interleaved rounds; medians with min and max"}
    if not args.resized_only:
        model_check(torch, hjd, ctx, dev)
        result["model_check"] = "Color == tests/color_model.py on 3 items of different sizes, float16"
        result["kernel_alone"] = kernel_alone(torch, hjd, ctx, dev, args.frames, args.rounds, args.warm_rounds, args.reps)
        for name, leg in result["kernel_alone"]["legs"].items():
            print(f"kernel {name:10s} {leg['ms_median']:9.4f} ms (median) {leg['ms_min']:9.4f} (min) {leg['ms_max']:9.4f} (max) "
                  f"x{leg['vs_copy_f16']} of the f16 copy", file=sys.stderr, flush=True)
    result["end_to_end"] = end_to_end(torch, hjd, ctx, dev, args.frames, args.rounds, args.warm_rounds, args.resized_only)
    for name, leg in result["end_to_end"]["legs"].items():
        print(f"e2e {name:10s} {leg['ms_median']:9.3f} ms (median) {leg['ms_min']:9.3f} (min) {leg['ms_max']:9.3f} (max)",
              file=sys.stderr, flush=True)
    if "holds" in result["end_to_end"]:
        print("holds", json.dumps(result["end_to_end"]["holds"]), file=sys.stderr, flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"color_ab": "ok", "file": os.path.relpath(args.out, REPO)}))


if __name__ == "__main__":
    main()

"""A/B of the filter stage on the GPU (backend.Conv and
GpuDecoder.decode_rgb_resized_aug()) against the route it replaces, one device,
same run.

    python tools/conv_ab.py [--frames 256] [--rounds 10] [--out profiles/conv_ab.json]
    python tools/conv_ab.py --probe      # one launch of the radius-11 Conv object of (a): for a counter collection

First, on a small case (three sources of different sizes, the three borders),
Conv's output must equal the numpy model's (tests/conv_model.py) bit for bit.

(a) The kernel alone.  `frames` x 3 x 224 x 224 random bytes to float16 with
ImageNet constants:
  conv_sharpness   Conv, conv_sharpness(1.7): radius 1, KEEP
  conv_gauss_r3    Conv, conv_gaussian(1.0): radius 3, REFLECT
  conv_gauss_r11   Conv, conv_gaussian(4.0): radius 11, REFLECT
  conv_identity    Conv, CONV_IDENTITY: the path without LDS
  tone_table       Tone with a solarize table: one launch that moves the same bytes
  copy_f16         a device copy of the bytes written (Tensor.copy_)
Device events around `--reps` back-to-back launches; the legs alternate inside
every round; medians with min and max.

(b) End to end.  `frames` q90 4:2:0 FHD JPEGs (bench.py's synthetic files, a
pool of distinct ones cycled), each with its own random-resized crop (8 % ..
100 % of the area, aspect 3/4 .. 4/3) and flip, every second one blurred
(conv_gaussian, sigma drawn from 0.1 .. 2.0, SimCLR's range) and the others
sharpened (conv_sharpness, factor drawn from 0.1 .. 1.9), to 224 x 224 float16
with ImageNet mean / std:
  conv     decode_rgb_resized_aug(size, rois=, flips=, convs=, dtype=float16, mean=, std=)
  resized  decode_rgb_resized(...) of the same crops to float16 without filters: what the stage adds to
  torch    the route it replaces: decode_rgb_resized() to uint8, then per image
           F.pad(mode="reflect") + conv2d with the filter's float taps (the
           sharpness images: the 3 x 3 smoothing kernel, the blend, the copied
           band), round, clamp and normalise in torch, rounded to half
Host clock around the call with a device synchronise before and inside the
window; interleaved rounds after untimed warm rounds.  Before timing, the
bytes of `conv` (a uint8 call) and of the torch route must agree within one
grey level (float32 sums against exact integers: a result next to a rounding
boundary may fall on either side), and the float16 results within one grey
level in normalised units.
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
    """Conv against tests/conv_model.py on a small case, bit for bit."""
    import conv_model
    shapes = [(37, 29), (300, 200), (5, 3)]
    filters = [hjd.conv_gaussian(4.0), hjd.conv_unsharp(1.0, 1.5, border=hjd.CONV_REPLICATE), hjd.conv_sharpness(0.3)]
    a, b = hjd.norm_constants(MEAN, STD)
    rng = np.random.default_rng(7)
    host = [rng.integers(0, 256, (3, h, w), dtype=np.uint8) for w, h in shapes]
    srcs = [torch.from_numpy(s).to(dev) for s in host]
    outs = [torch.zeros(s.shape, dtype=torch.float16, device=dev) for s in host]
    op = hjd.Conv(ctx, srcs, outs, filters=filters, normalize=(a, b))
    op.launch(torch.cuda.current_stream())
    torch.cuda.synchronize()
    op.close()
    for k in range(3):
        exp = conv_model.conv(host[k], conv_model.from_numpy(filters[k]), np.float16, tuple(float(v) for v in a),
                              tuple(float(v) for v in b))
        if not np.array_equal(outs[k].cpu().numpy().view(np.uint16), exp):
            raise SystemExit(f"item {k}: Conv differs from the model")


def kernel_alone(torch, hjd, ctx, dev, nf, rounds, warm_rounds, reps, probe=False):
    gen = torch.Generator(device=dev).manual_seed(5)
    src = torch.randint(0, 256, (nf, 3, OUT, OUT), dtype=torch.uint8, device=dev, generator=gen)
    srcs = [src[i] for i in range(nf)]
    norm = hjd.norm_constants(MEAN, STD)
    stream = torch.cuda.current_stream()
    filters = {"conv_sharpness": hjd.conv_sharpness(1.7), "conv_gauss_r3": hjd.conv_gaussian(1.0),
               "conv_gauss_r11": hjd.conv_gaussian(4.0), "conv_identity": hjd.CONV_IDENTITY}
    radii = {name: [int(f["rx"]), int(f["ry"])] for name, f in filters.items()}
    if radii["conv_gauss_r3"] != [3, 3] or radii["conv_gauss_r11"] != [11, 11]:
        raise SystemExit(f"the legs' radii are {radii}")
    if probe:
        out = torch.zeros((nf, 3, OUT, OUT), dtype=torch.float16, device=dev)
        op = hjd.Conv(ctx, srcs, out, filters=filters["conv_gauss_r11"], normalize=norm)
        op.launch(stream)
        torch.cuda.synchronize()
        op.close()
        return {"frames": nf, "launched_once": ["conv_gauss_r11"]}
    outs = {name: torch.zeros((nf, 3, OUT, OUT), dtype=torch.float16, device=dev) for name in list(filters) + ["tone_table"]}
    copy_f16 = torch.empty_like(outs["tone_table"])
    ops = {name: hjd.Conv(ctx, srcs, outs[name], filters=f, normalize=norm) for name, f in filters.items()}
    ops["tone_table"] = hjd.Tone(ctx, srcs, outs["tone_table"], curves=hjd.tone_curve(solarize=128), normalize=norm)
    legs = {"copy_f16": lambda: copy_f16.copy_(outs["tone_table"])}
    legs.update({name: (lambda op=op: op.launch(stream)) for name, op in ops.items()})

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
    res = {"frames": nf, "size": [OUT, OUT], "dtype": "float16", "launches_per_sample": reps, "radii": radii,
           "bytes_read": src.numel(), "bytes_written": copy_f16.numel() * 2,
           "timing": "device events around the back-to-back launches, per launch",
           "legs": {name: stats(v) for name, v in ms.items()}}
    L = res["legs"]
    for leg in L.values():
        leg["vs_copy_f16"] = round(leg["ms_median"] / L["copy_f16"]["ms_median"], 4)
        leg["vs_tone_table"] = round(leg["ms_median"] / L["tone_table"]["ms_median"], 4)
    for op in ops.values():
        op.close()
    del src, srcs, outs, copy_f16
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


def torch_conv(torch, u8, filters):
    """The bytes of the filter stage on a (n, 3, h, w) uint8 batch, in torch, image by image: the
    record's taps / 4096 as float32 kernels, reflect padding (replicate for a KEEP record, whose band
    is then copied), conv2d per channel, the blend, round half up, clamp."""
    import torch.nn.functional as F
    out = torch.empty_like(u8)
    for i, f in enumerate(filters):
        rx, ry = int(f["rx"]), int(f["ry"])
        x = u8[i].float().unsqueeze(0)   # (1, 3, h, w)
        kh = torch.tensor(f["kh"][:2 * rx + 1].astype(np.float32) / 4096.0, device=u8.device)
        kv = torch.tensor(f["kv"][:2 * ry + 1].astype(np.float32) / 4096.0, device=u8.device)
        k2 = (kv.view(-1, 1) * kh.view(1, -1)).expand(3, 1, 2 * ry + 1, 2 * rx + 1).contiguous()
        keep = int(f["border"]) == 0
        pad = F.pad(x, (rx, rx, ry, ry), mode="replicate" if keep else "reflect") if rx or ry else x
        s = F.conv2d(pad, k2, groups=3)
        y = torch.floor((float(f["a"]) / 4096.0) * x + (float(f["b"]) / 4096.0) * s + 0.5).clamp_(0, 255)
        if keep and (rx or ry):
            band = torch.ones_like(y, dtype=torch.bool)
            band[..., ry:y.shape[2] - ry, rx:y.shape[3] - rx] = False
            y = torch.where(band, x, y)
        out[i] = y[0].to(torch.uint8)
    return out


def end_to_end(torch, hjd, ctx, dev, nf, rounds, warm_rounds):
    import bench
    pool = bench.encode_pool(W, H, hjd.YUV420, min(POOL, nf), seed0=9400)
    datas = [pool[i % len(pool)] for i in range(nf)]
    rng = np.random.default_rng(11)
    rois = crops(rng, nf)
    flips = [bool(v) for v in rng.integers(0, 2, nf)]
    info = hjd.parse(datas[0])
    gd = hjd.GpuDecoder(ctx, nf, 2 * sum(map(len, datas)), nf * info.nblocks)
    last = {}
    convs = [hjd.conv_gaussian(float(rng.uniform(0.1, 2.0)), ksize=23) if i % 2 == 0 else
             hjd.conv_sharpness(float(rng.uniform(0.1, 1.9))) for i in range(nf)]
    a_np, b_np = hjd.norm_constants(MEAN, STD)
    a32 = torch.tensor(a_np, device=dev).view(1, 3, 1, 1)
    b32 = torch.tensor(b_np, device=dev).view(1, 3, 1, 1)

    def leg_resized():
        last["resized"] = gd.decode_rgb_resized(datas, (OUT, OUT), flips=flips, rois=rois, dtype=torch.float16,
                                                mean=MEAN, std=STD)
        gd.sync()

    def leg_conv():
        last["conv"] = gd.decode_rgb_resized_aug(datas, (OUT, OUT), flips=flips, rois=rois, convs=convs,
                                                 dtype=torch.float16, mean=MEAN, std=STD)
        gd.sync()

    def leg_torch():
        u8 = gd.decode_rgb_resized(datas, (OUT, OUT), flips=flips, rois=rois)
        gd.sync()
        last["torch_u8"] = torch_conv(torch, u8, convs)
        last["torch"] = torch.addcmul(b32, last["torch_u8"].float(), a32).half()

    jobs = [("resized", leg_resized), ("conv", leg_conv), ("torch", leg_torch)]
    for _ in range(max(1, warm_rounds)):
        for _, job in jobs:
            job()
    torch.cuda.synchronize()
    conv_u8 = gd.decode_rgb_resized_aug(datas, (OUT, OUT), flips=flips, rois=rois, convs=convs)
    gd.sync()
    d8 = (conv_u8.int() - last["torch_u8"].int()).abs()
    if int(d8.max()) > 1:
        raise SystemExit(f"the filter decode and the torch route differ by {int(d8.max())} grey levels")
    diff = float((last["conv"].float() - last["torch"].float()).abs().max())
    level = float(max(a_np)) * 1.01 + 2.0 ** -9   # one grey level in normalised units, and a step of half precision
    if diff > level:
        raise SystemExit(f"the float16 results differ by {diff} (one grey level is {level})")
    res = {"frames": nf, "width": W, "height": H, "out": [OUT, OUT], "distinct_files": len(pool),
           "jpeg_bytes": sum(map(len, datas)), "dtype": "float16", "crop_area": [0.08, 1.0],
           "decoded_pixel_fraction": round(sum(r[2] * r[3] for r in rois) / (nf * W * H), 4),
           "convs": "even images blurred (conv_gaussian, sigma 0.1..2.0, ksize 23 before trimming), odd ones sharpened "
                    "(conv_sharpness, factor 0.1..1.9)",
           "radii": sorted({int(f["rx"]) for f in convs}),
           "max_abs_diff_u8_vs_torch": int(d8.max()),
           "share_of_bytes_differing_from_torch": round(float((d8 != 0).float().mean()), 6),
           "max_abs_diff_float16": diff,
           "timing": "host clock around the call, a device synchronise before and inside the window"}

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
    res["holds"] = {"conv_vs_torch": round(L["conv"]["ms_median"] / L["torch"]["ms_median"], 4),
                    "conv_minus_resized_ms": round(L["conv"]["ms_median"] - L["resized"]["ms_median"], 4),
                    "conv_below_torch": L["conv"]["ms_median"] < L["torch"]["ms_median"]}
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
    ap.add_argument("--probe", action="store_true",
                    help="launch the radius-11 object of (a) once and stop: the run a counter collection wraps")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "conv_ab.json"))
    args = ap.parse_args()
    import torch
    import ocljpegdecoder_amd as hjd
    if not torch.cuda.is_available():
        raise SystemExit("conv_ab needs a GPU: no timing is taken without one")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = hjd.Context(0)
    if args.probe:
        print(json.dumps({"conv_ab": "probe", **kernel_alone(torch, hjd, ctx, dev, args.frames, 0, 0, 1, probe=True)}))
        ctx.close()
        return
    result = {"tool": "tools/conv_ab.py", "utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
              "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "frames": args.frames,
              "rounds": args.rounds, "warm_rounds": args.warm_rounds, "mean": list(MEAN), "std": list(STD),
              "method": "untimed interleaved warm rounds of every leg, then interleaved rounds; medians with min and max"}
    model_check(torch, hjd, ctx, dev)
    result["model_check"] = "Conv == tests/conv_model.py on 3 items of different sizes, the three borders, float16"
    result["kernel_alone"] = kernel_alone(torch, hjd, ctx, dev, args.frames, args.rounds, args.warm_rounds, args.reps)
    for name, leg in result["kernel_alone"]["legs"].items():
        print(f"kernel {name:18s} {leg['ms_median']:9.4f} ms (median) {leg['ms_min']:9.4f} (min) {leg['ms_max']:9.4f} (max) "
              f"x{leg['vs_copy_f16']} of the f16 copy", file=sys.stderr, flush=True)
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
    print(json.dumps({"conv_ab": "ok", "file": os.path.relpath(args.out, REPO)}))


if __name__ == "__main__":
    main()

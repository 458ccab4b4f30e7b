"""A/B of the resized decode (GpuDecoder.decode_rgb_resized: JPEG bytes -> one
(N, 3, 224, 224) float16 batch, two launches after the entropy decode) against
the route it replaces, one device, same run.

    python tools/resize_ab.py [--frames 256] [--rounds 10] [--out profiles/resize_ab.json]

Workload: `frames` q90 4:2:0 JPEGs (bench.py's synthetic files, a pool of
distinct ones cycled) of 1920x1080, then of 3840x2160; one seeded
random-resized crop per image (8-100 % of the area, aspect ratio 3/4-4/3,
log-uniform, as torchvision's RandomResizedCrop draws them) and a seeded flip
for every second image on average; the decode scale is resize_scale() of the
smallest crop, and the crops are taken on that scale's grid.  Output 224x224,
float16, ImageNet mean / std.

Legs (interleaved rounds after untimed warm rounds of every leg; each timed
window is a host clock around the call and a device synchronise, because the
route that is replaced is made of hundreds of small launches whose cost is on
the host):
  a           decode_rgb_resized(size=, flips=, rois=, scale=, dtype=float16, mean=, std=)
  c           decode_rgb(rois=, scale=) into a list of uint8 crops: the decode alone
  b_*         the route a replaces: leg c, then per image interpolate(bilinear,
              antialias=False), flip and normalise into a preallocated batch,
              every spelling in SPELLINGS; the fastest (lowest median) is the
              one a is compared with, and its name is recorded
  resize      the resize kernel alone (backend.Resize over leg c's crops), by
              device events, with its algorithmic bytes (crop bytes read +
              batch bytes written) as a fraction of 8 TB/s

`holds`: a's median below the fastest b's median (the condition).  Recorded
beside it: the ratio, and a against c (what the resize adds to the decode).
Before timing, a must equal the resize kernel alone on leg c's crops bit for
bit, and agree with the fastest b to 0.02 in normalised units (0.75 of a byte
step is 0.0131 for the smallest std; half precision adds 0.002).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
OUT = (224, 224)   # (h, w)
POOL = 8
HBM_BYTES_PER_MS = 8e9   # 8 TB/s


def random_resized_crops(rng, n, w, h):
    """(x, y, cw, ch) per image on the full-size grid: area 8-100 %, aspect 3/4-4/3 (log-uniform)."""
    rois = []
    while len(rois) < n:
        area = rng.uniform(0.08, 1.0) * w * h
        ratio = math.exp(rng.uniform(math.log(3 / 4), math.log(4 / 3)))
        cw, ch = int(round(math.sqrt(area * ratio))), int(round(math.sqrt(area / ratio)))
        if 0 < cw <= w and 0 < ch <= h:
            rois.append((int(rng.integers(0, w - cw + 1)), int(rng.integers(0, h - ch + 1)), cw, ch))
    return rois


def on_scaled_grid(rois, w, h, s):
    sw, sh = -(-w // s), -(-h // s)
    out = []
    for x, y, cw, ch in rois:
        x0, y0 = x // s, y // s
        x1, y1 = min(sw, -(-(x + cw) // s)), min(sh, -(-(y + ch) // s))
        out.append((x0, y0, max(1, x1 - x0), max(1, y1 - y0)))
    return out


def spellings(torch, F):
    """Ways to take one uint8 crop (3, h, w) to the normalised float16 (3, 224, 224) slot `out`."""
    def f32_interp(c, flip, a32, b32, a16, b16, out):
        y = F.interpolate(c[None].float(), size=OUT, mode="bilinear", align_corners=False, antialias=False)
        z = torch.addcmul(b32, y, a32)
        out.copy_((z.flip(-1) if flip else z)[0])

    def f16_interp(c, flip, a32, b32, a16, b16, out):
        y = F.interpolate(c[None].half(), size=OUT, mode="bilinear", align_corners=False, antialias=False)
        z = torch.addcmul(b16, y, a16)
        out.copy_((z.flip(-1) if flip else z)[0])

    def f16_interp_out(c, flip, a32, b32, a16, b16, out):
        y = F.interpolate(c[None].half(), size=OUT, mode="bilinear", align_corners=False, antialias=False)
        if flip:
            y = y.flip(-1)
        torch.addcmul(b16, y, a16, out=out[None])

    return [("f32_interp_addcmul_copy", f32_interp), ("f16_interp_addcmul_copy", f16_interp),
            ("f16_interp_addcmul_out", f16_interp_out)]


def run_size(torch, hjd, ctx, dev, w, h, nf, rounds, warm_rounds):
    import torch.nn.functional as F
    import bench
    pool = bench.encode_pool(w, h, hjd.YUV420, min(POOL, nf), seed0=9100 + w)
    datas = [pool[i % len(pool)] for i in range(nf)]
    info = hjd.parse(datas[0])
    rng = np.random.default_rng(20240 + w)
    full_rois = random_resized_crops(rng, nf, w, h)
    flips = [bool(v) for v in rng.integers(0, 2, nf)]
    scale = min(hjd.resize_scale(r[2], r[3], OUT[1], OUT[0]) for r in full_rois)
    rois = on_scaled_grid(full_rois, w, h, scale)
    a_np, b_np = hjd.norm_constants(MEAN, STD)
    a32 = torch.tensor(a_np, device=dev).view(1, 3, 1, 1)
    b32 = torch.tensor(b_np, device=dev).view(1, 3, 1, 1)
    a16, b16 = a32.half(), b32.half()
    gd = hjd.GpuDecoder(ctx, nf, 2 * sum(map(len, datas)), nf * info.nblocks)
    batch_a = torch.zeros((nf, 3) + OUT, dtype=torch.float16, device=dev)
    batch_b = torch.zeros((nf, 3) + OUT, dtype=torch.float16, device=dev)
    kw = dict(dtype=torch.float16, mean=MEAN, std=STD)

    def leg_a():
        gd.decode_rgb_resized(datas, OUT, flips=flips, out=batch_a, scale=scale, rois=rois, **kw)
        gd.sync()

    def leg_c():
        crops = gd.decode_rgb(datas, scale=scale, rois=rois)
        gd.sync()
        return crops

    def leg_b(fn):
        crops = leg_c()
        for i, c in enumerate(crops):
            fn(c, flips[i], a32, b32, a16, b16, batch_b[i])

    usable = []
    probe = torch.zeros((3, 40, 50), dtype=torch.uint8, device=dev)
    for name, fn in spellings(torch, F):   # a spelling this torch refuses is left out, and named
        try:
            fn(probe, True, a32, b32, a16, b16, batch_b[0])
            usable.append((name, fn))
        except Exception as e:   # noqa: BLE001
            print(f"spelling {name}: not usable ({type(e).__name__}: {str(e)[:80]})", file=sys.stderr, flush=True)
    if not usable:
        raise SystemExit("no spelling of the replaced route works")
    jobs = [("a", leg_a), ("c", leg_c)] + [(f"b_{name}", (lambda fn=fn: leg_b(fn))) for name, fn in usable]
    for _ in range(max(1, warm_rounds)):
        for _, job in jobs:
            job()
    torch.cuda.synchronize()

    # the resize kernel alone over leg c's crops
    crops = leg_c()
    torch.cuda.synchronize()
    alone = torch.zeros((nf, 3) + OUT, dtype=torch.float16, device=dev)
    rz = hjd.Resize(ctx, crops, alone, flips=flips, normalize=(a_np, b_np))
    stream = torch.cuda.current_stream()
    rz.launch(stream)
    torch.cuda.synchronize()
    if not torch.equal(alone.view(torch.int16), batch_a.view(torch.int16)):
        raise SystemExit("the resized decode differs from the resize kernel alone on the decoded crops")

    def timed_wall(job):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        job()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def timed_events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    ms = {name: [] for name, _ in jobs}
    ms["resize"] = []
    agree = {}
    for r in range(rounds):
        for name, job in jobs:
            ms[name].append(timed_wall(job))
            if r == 0 and name.startswith("b_"):
                agree[name] = float((batch_b.float() - batch_a.float()).abs().max())
        ms["resize"].append(timed_events(lambda: rz.launch(stream)))
    rz.close()

    def stats(v):
        return {"ms_min": round(min(v), 4), "ms_median": round(statistics.median(v), 4), "ms_max": round(max(v), 4),
                "ms_rounds": [round(t, 4) for t in v]}

    crop_bytes = sum(3 * r[2] * r[3] for r in rois)
    batch_bytes = batch_a.numel() * batch_a.element_size()
    res = {"width": w, "height": h, "frames": nf, "distinct_files": len(pool), "jpeg_bytes": sum(map(len, datas)),
           "scale": scale, "crop_px_min": min(r[2] * r[3] for r in rois), "crop_px_max": max(r[2] * r[3] for r in rois),
           "crop_bytes": crop_bytes, "batch_bytes": batch_bytes, "flipped": sum(flips),
           "legs": {name: stats(v) for name, v in ms.items()}, "max_abs_diff_vs_a": agree}
    rk = res["legs"]["resize"]
    rk["timing"] = "device events around the launch"
    rk["algorithmic_bytes"] = crop_bytes + batch_bytes
    rk["fraction_of_8TBps"] = round((crop_bytes + batch_bytes) / rk["ms_median"] / HBM_BYTES_PER_MS, 4)
    best = min((res["legs"][n]["ms_median"], n) for n in ms if n.startswith("b_"))
    if agree[best[1]] > 0.02:
        raise SystemExit(f"leg a and {best[1]} differ by {agree[best[1]]} in normalised units")
    a, c = res["legs"]["a"], res["legs"]["c"]
    res["holds"] = {"a_ms_median": a["ms_median"], "a_ms_max": a["ms_max"], "b": best[1], "b_ms_median": best[0],
                    "a_vs_b": round(a["ms_median"] / best[0], 4), "a_below_b": a["ms_median"] < best[0],
                    "c_ms_median": c["ms_median"], "a_vs_c": round(a["ms_median"] / c["ms_median"], 4),
                    "a_minus_c_ms": round(a["ms_median"] - c["ms_median"], 4)}
    gd.close()
    del batch_a, batch_b, alone, crops
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warm-rounds", type=int, default=2, help="untimed interleaved rounds before the timed ones")
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "resize_ab.json"))
    args = ap.parse_args()
    import torch
    import ocljpegdecoder_amd as hjd
    if not torch.cuda.is_available():
        raise SystemExit("resize_ab needs a GPU: no timing is taken without one")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = hjd.Context(0)
    result = {"tool": "tools/resize_ab.py", "utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
              "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "frames": args.frames,
              "rounds": args.rounds, "warm_rounds": args.warm_rounds, "out_size": list(OUT), "dtype": "float16",
              "mean": list(MEAN), "std": list(STD),
              "method": "untimed interleaved warm rounds of every leg, then interleaved rounds; legs a, b_*, c: host "
                        "clock around the call, a device synchronise before and inside the window; resize: device "
                        "events around the launch",
              "sizes": {}}
    for spec in args.sizes.split(","):
        w, h = (int(v) for v in spec.split("x"))
        r = run_size(torch, hjd, ctx, dev, w, h, args.frames, args.rounds, args.warm_rounds)
        result["sizes"][spec] = r
        for name, leg in r["legs"].items():
            print(f"{spec} {name:28s} {leg['ms_median']:9.3f} ms (median) {leg['ms_max']:9.3f} (max)", file=sys.stderr,
                  flush=True)
        print(spec, "holds", json.dumps(r["holds"]), file=sys.stderr, flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"resize_ab": "ok", "file": os.path.relpath(args.out, REPO)}))


if __name__ == "__main__":
    main()

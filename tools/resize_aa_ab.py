"""A/B of the antialiased resized decode (GpuDecoder.decode_rgb_resized(...,
antialias=True): JPEG bytes -> one (N, 3, 224, 224) float16 batch, three
launches after the entropy decode) against the route it replaces, one device,
same run.  Workload and method are tools/resize_ab.py's.

    python tools/resize_aa_ab.py [--frames 256] [--rounds 10] [--out profiles/resize_aa_ab.json]

Workload: `frames` q90 4:2:0 JPEGs of 1920x1080, then of 3840x2160; one seeded
random-resized crop per image and a seeded flip; the decode scale is
resize_scale() of the smallest crop, so the larger crops are reduced 2.5-6x per
axis by the resize itself.  Output 224x224, float16, ImageNet mean / std.

Legs (interleaved rounds after untimed warm rounds of every leg; each timed
window is a host clock around the call and a device synchronise):
  a_aa        decode_rgb_resized(..., antialias=True)
  a           the same call with antialias=False (plain bilinear)
  b_aa_*      decode_rgb(rois=, scale=), then per image interpolate(bilinear,
              antialias=True), flip and addcmul into a preallocated batch, in
              float16 and in float32; the faster (lower median) is the one
              a_aa is compared with, and its name is recorded
  aa_h, aa_v  the two kernels alone (backend.Resize(antialias=True) over the
              decoded crops, one pass per launch), by device events, with the
              bytes each moves

`holds`: a_aa's median below the faster b_aa's median (the condition).
Recorded beside it: a_aa - a, the kernels' times, the intermediate's bytes, and
the largest difference of a_aa from torch's float32 antialiased result in
normalised units, which must stay within one byte step over the smallest std
(the model's distance from the real-valued filter) plus the two half roundings.
Before timing, a_aa must equal Resize(antialias=True) alone on the decoded
crops bit for bit.
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
sys.path.insert(0, os.path.join(REPO, "tools"))

from resize_ab import HBM_BYTES_PER_MS, MEAN, OUT, POOL, STD, on_scaled_grid, random_resized_crops  # noqa: E402

# 1.0 byte (tests/test_resize_aa_cpu.py) in normalised units, + half's rounding
# of a_aa and of the reference batch (values below 4: spacing 2^-9 each)
AGREE_BOUND = 1.0 / (255.0 * min(STD)) + 2 * 2.0 ** -10


def spellings(torch, F):
    """interpolate(antialias=True) of one uint8 crop (3, h, w) into the normalised float16 slot `out`."""
    def make(dt):
        def fn(c, flip, a, b, out):
            y = F.interpolate(c[None].to(dt), size=OUT, mode="bilinear", align_corners=False, antialias=True)
            z = torch.addcmul(b[dt], y, a[dt])
            out.copy_((z.flip(-1) if flip else z)[0])
        return fn
    return [("b_aa_f16", make(torch.float16)), ("b_aa_f32", make(torch.float32))]


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
    a = {torch.float32: a32, torch.float16: a32.half()}
    b = {torch.float32: b32, torch.float16: b32.half()}
    gd = hjd.GpuDecoder(ctx, nf, 2 * sum(map(len, datas)), nf * info.nblocks)
    batch_aa = torch.zeros((nf, 3) + OUT, dtype=torch.float16, device=dev)
    batch_a = torch.zeros((nf, 3) + OUT, dtype=torch.float16, device=dev)
    batch_b = torch.zeros((nf, 3) + OUT, dtype=torch.float16, device=dev)
    kw = dict(dtype=torch.float16, mean=MEAN, std=STD)

    def leg_a_aa():
        gd.decode_rgb_resized(datas, OUT, flips=flips, out=batch_aa, scale=scale, rois=rois, antialias=True, **kw)
        gd.sync()

    def leg_a():
        gd.decode_rgb_resized(datas, OUT, flips=flips, out=batch_a, scale=scale, rois=rois, **kw)
        gd.sync()

    def decode_crops():
        crops = gd.decode_rgb(datas, scale=scale, rois=rois)
        gd.sync()
        return crops

    def leg_b(fn):
        for i, c in enumerate(decode_crops()):
            fn(c, flips[i], a, b, batch_b[i])

    usable = []
    probe = torch.zeros((3, 400, 500), dtype=torch.uint8, device=dev)
    for name, fn in spellings(torch, F):   # a spelling this torch refuses is left out, and named
        try:
            fn(probe, True, a, b, batch_b[0])
            usable.append((name, fn))
        except Exception as e:   # noqa: BLE001
            print(f"spelling {name}: not usable ({type(e).__name__}: {str(e)[:80]})", file=sys.stderr, flush=True)
    if not usable:
        raise SystemExit("no spelling of the replaced route works")
    jobs = [("a_aa", leg_a_aa), ("a", leg_a)] + [(name, (lambda fn=fn: leg_b(fn))) for name, fn in usable]
    for _ in range(max(1, warm_rounds)):
        for _, job in jobs:
            job()
    torch.cuda.synchronize()

    # the two kernels alone over the decoded crops
    crops = decode_crops()
    torch.cuda.synchronize()
    alone = torch.zeros((nf, 3) + OUT, dtype=torch.float16, device=dev)
    rz = hjd.Resize(ctx, crops, alone, flips=flips, normalize=(a_np, b_np), antialias=True)
    stream = torch.cuda.current_stream()
    rz.launch(stream)
    torch.cuda.synchronize()
    if not torch.equal(alone.view(torch.int16), batch_aa.view(torch.int16)):
        raise SystemExit("the antialiased resized decode differs from Resize(antialias=True) alone on the decoded crops")
    # against torch's own antialiased result, computed in float32
    f32 = dict(spellings(torch, F))["b_aa_f32"]
    for i, c in enumerate(crops):
        f32(c, flips[i], a, b, batch_b[i])
    torch.cuda.synchronize()
    agree = float((batch_b.float() - batch_aa.float()).abs().max())
    if agree > AGREE_BOUND:
        raise SystemExit(f"a_aa differs from torch's antialiased result by {agree} in normalised units "
                         f"(bound {AGREE_BOUND})")

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
    ms["aa_h"], ms["aa_v"] = [], []
    for _ in range(rounds):
        for name, job in jobs:
            ms[name].append(timed_wall(job))
        ms["aa_h"].append(timed_events(lambda: rz.launch_pass(0, stream)))
        ms["aa_v"].append(timed_events(lambda: rz.launch_pass(1, stream)))
    rz.close()

    def stats(v):
        return {"ms_min": round(min(v), 4), "ms_median": round(statistics.median(v), 4), "ms_max": round(max(v), 4),
                "ms_rounds": [round(t, 4) for t in v]}

    crop_bytes = sum(3 * r[2] * r[3] for r in rois)
    mid_bytes = sum(3 * ((OUT[1] + 3) // 4 * 4) * r[3] for r in rois)
    batch_bytes = batch_aa.numel() * batch_aa.element_size()
    res = {"width": w, "height": h, "frames": nf, "distinct_files": len(pool), "jpeg_bytes": sum(map(len, datas)),
           "scale": scale, "crop_px_min": min(r[2] * r[3] for r in rois), "crop_px_max": max(r[2] * r[3] for r in rois),
           "reduction_max": round(max(max(r[2] / OUT[1], r[3] / OUT[0]) for r in rois), 3),
           "crop_bytes": crop_bytes, "intermediate_bytes": mid_bytes, "batch_bytes": batch_bytes, "flipped": sum(flips),
           "legs": {name: stats(v) for name, v in ms.items()},
           "max_abs_diff_a_aa_vs_torch_f32": agree, "max_abs_diff_bound": AGREE_BOUND}
    for leg, moved in (("aa_h", crop_bytes + mid_bytes), ("aa_v", mid_bytes + batch_bytes)):
        k = res["legs"][leg]
        k["timing"] = "device events around the one launch"
        k["algorithmic_bytes"] = moved
        k["fraction_of_8TBps"] = round(moved / k["ms_median"] / HBM_BYTES_PER_MS, 4)
    best = min((res["legs"][n]["ms_median"], n) for n, _ in usable)
    a_aa, a_ = res["legs"]["a_aa"], res["legs"]["a"]
    res["holds"] = {"a_aa_ms_median": a_aa["ms_median"], "a_aa_ms_max": a_aa["ms_max"], "b_aa": best[1],
                    "b_aa_ms_median": best[0], "a_aa_vs_b_aa": round(a_aa["ms_median"] / best[0], 4),
                    "a_aa_below_b_aa": a_aa["ms_median"] < best[0], "a_ms_median": a_["ms_median"],
                    "a_aa_minus_a_ms": round(a_aa["ms_median"] - a_["ms_median"], 4)}
    gd.close()
    del batch_aa, batch_a, batch_b, alone, crops
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warm-rounds", type=int, default=2, help="untimed interleaved rounds before the timed ones")
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "resize_aa_ab.json"))
    args = ap.parse_args()
    import torch
    import ocljpegdecoder_amd as hjd
    if not torch.cuda.is_available():
        raise SystemExit("resize_aa_ab needs a GPU: no timing is taken without one")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = hjd.Context(0)
    result = {"tool": "tools/resize_aa_ab.py", "utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
              "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "frames": args.frames,
              "rounds": args.rounds, "warm_rounds": args.warm_rounds, "out_size": list(OUT), "dtype": "float16",
              "mean": list(MEAN), "std": list(STD),
              "method": "untimed interleaved warm rounds of every leg, then interleaved rounds; legs a_aa, a, b_aa_*: "
                        "host clock around the call, a device synchronise before and inside the window; aa_h, aa_v: "
                        "device events around one launch",
              "sizes": {}}
    for spec in args.sizes.split(","):
        w, h = (int(v) for v in spec.split("x"))
        r = run_size(torch, hjd, ctx, dev, w, h, args.frames, args.rounds, args.warm_rounds)
        result["sizes"][spec] = r
        for name, leg in r["legs"].items():
            print(f"{spec} {name:12s} {leg['ms_median']:9.3f} ms (median) {leg['ms_max']:9.3f} (max)", file=sys.stderr,
                  flush=True)
        print(spec, "holds", json.dumps(r["holds"]), file=sys.stderr, flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"resize_aa_ab": "ok", "file": os.path.relpath(args.out, REPO)}))


if __name__ == "__main__":
    main()

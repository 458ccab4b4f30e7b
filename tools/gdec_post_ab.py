"""A/B of two builds of the library on the decoder's host paths, for a change
that must leave speed as it is: build/variants/<parent>/libhjd.so against the
product library, alternating, each measurement in a child process.

    python tools/build_native.py --variant parent      (at the parent commit)
    python tools/gdec_post_ab.py [--parent parent] [--reps 5] [--out profiles/gdec_post_refactor.json]

Per repetition and library:
  (a) tools/fhd_host_times.py's loop: one FHD q90 image, decode + sync, pageable
      bytes; host us per call (wait, stage, issue: HJD_GDEC_HOST_TIMES) and ms/image
  (b) the library's own leg of tools/resize_ab.py, resize_aa_ab.py, orient_ab.py
      and warp_ab.py, as those tools build it: 256 FHD files to 224 x 224 float16
      (orient_ab's: to oriented full frames), host clock around call + sync,
      median of --rounds after --warm-rounds; and the 256-frame decoder's host us
      per call over these legs (batch_*_us)
  (c) bench.py --gpus 1 (--bench-args), its "value" and its FHD JPEG leg

Criterion per number: the product's median over the repetitions lies within the
parent's own min..max over its repetitions, widened by 2 % (for times: not above
max * 1.02; for rates: not below min * 0.98).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def child(nf, rounds, warm, n_latency):
    """Measure (a) and (b) with the library HJD_LIB names; one JSON line on stdout."""
    import numpy as np
    import torch

    import bench
    import ocljpegdecoder_amd as hjd
    import orient_ab
    import resize_ab
    W, H, OUT = 1920, 1080, (224, 224)
    ctx = hjd.Context(0)
    dev = torch.device("cuda", 0)
    res = {}

    # (a)
    data = bench.encode_pool(W, H, 1, 1, seed0=4242)[0]
    info = hjd.parse(data)
    out = torch.empty((H, W), dtype=torch.int32, device="cuda")
    gd = hjd.GpuDecoder(ctx, 1, len(data), info.nblocks)
    for _ in range(20):
        gd.decode([data], [out])
        gd.sync()
    gd.close()
    gd = hjd.GpuDecoder(ctx, 1, len(data), info.nblocks)
    t = time.perf_counter()
    for _ in range(n_latency):
        gd.decode([data], [out])
        gd.sync()
    res["fhd_ms_per_image"] = (time.perf_counter() - t) / n_latency * 1e3
    gd.close()   # prints the host times to stderr: the parent process reads them

    def timed(job):
        for _ in range(warm):
            job()
        ms = []
        for _ in range(rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            job()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms)

    kw = dict(dtype=torch.float16, mean=MEAN, std=STD)
    # resize_ab / resize_aa_ab
    pool = bench.encode_pool(W, H, hjd.YUV420, 8, seed0=9100 + W)
    datas = [pool[i % len(pool)] for i in range(nf)]
    rng = np.random.default_rng(20240 + W)
    full_rois = resize_ab.random_resized_crops(rng, nf, W, H)
    flips = [bool(v) for v in rng.integers(0, 2, nf)]
    scale = min(hjd.resize_scale(r[2], r[3], OUT[1], OUT[0]) for r in full_rois)
    rois = resize_ab.on_scaled_grid(full_rois, W, H, scale)
    gd = hjd.GpuDecoder(ctx, nf, 2 * sum(map(len, datas)), nf * info.nblocks)
    batch = torch.zeros((nf, 3) + OUT, dtype=torch.float16, device=dev)

    def resized(aa):
        gd.decode_rgb_resized(datas, OUT, flips=flips, out=batch, scale=scale, rois=rois, antialias=aa, **kw)
        gd.sync()

    res["resized_ms"] = timed(lambda: resized(False))
    res["resized_aa_ms"] = timed(lambda: resized(True))
    # warp_ab
    rng = np.random.default_rng(11)
    angles, zooms = rng.uniform(-30.0, 30.0, nf), rng.uniform(1.0, 2.0, nf)
    xf = [hjd.warp_xform(W, H, 224, 224, angle=float(a), zoom=float(z)) for a, z in zip(angles, zooms)]

    keep = []

    def warped():
        keep[:] = [gd.decode_rgb_warped(datas, OUT, xf, **kw)]
        gd.sync()

    res["warped_ms"] = timed(warped)
    # orient_ab
    mixed = [orient_ab.tagged(d, 6 if i % 8 == 7 else 1) for i, d in enumerate(datas)]

    def oriented():
        keep[:] = [gd.decode_rgb_oriented(mixed, apply_exif_orientation=True, **kw)]
        gd.sync()

    res["oriented_ms"] = timed(oriented)
    gd.close()
    print(json.dumps(res), flush=True)


def run_child(lib, args):
    env = dict(os.environ, HJD_GDEC_HOST_TIMES="1")
    env.pop("HJD_LIB", None)
    if lib:
        env["HJD_LIB"] = lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--frames", str(args.frames), "--rounds",
                        str(args.rounds), "--warm-rounds", str(args.warm_rounds), "--n", str(args.n)],
                       env=env, capture_output=True, text=True, timeout=600)
    if p.returncode:
        raise SystemExit(f"{lib or 'product'}: exit {p.returncode}\n{p.stderr[-2000:]}")
    res = json.loads(p.stdout.strip().splitlines()[-1])
    # "... wait_staging W stage S issue I" per decoder closed: (a)'s warm one, (a)'s timed one, (b)'s 256-frame one
    lines = [ln.split() for ln in p.stderr.splitlines() if "hjd_gdec host us/call" in ln]
    for name, line in (("fhd", lines[1]), ("batch", lines[2])):
        for key in ("wait_staging", "stage", "issue"):
            res[f"{name}_{key}_us"] = float(line[line.index(key) + 1])
    return res


def run_bench(lib, args):
    env = dict(os.environ)
    env.pop("HJD_LIB", None)
    if lib:
        env["HJD_LIB"] = lib
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1"] + args.bench_args.split(),
                       env=env, capture_output=True, text=True, timeout=900, cwd=REPO)
    if p.returncode:
        raise SystemExit(f"bench.py, {lib or 'product'}: exit {p.returncode}\n{p.stderr[-2000:]}")
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    res = {"bench_value_Mpx_s": line["value"]}
    fj = (line.get("summary") or {}).get("fhd420_jpeg_ms_per_image")
    if fj and "ms" in fj:
        res["bench_fhd420_jpeg_ms_per_image"] = fj["ms"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent", default="parent", help="build/variants/<name>/libhjd.so")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warm-rounds", type=int, default=3)
    ap.add_argument("--n", type=int, default=1000, help="(a): timed calls")
    ap.add_argument("--bench-args", default="--steps 20 --warmup 3")
    ap.add_argument("--skip-bench", action="store_true")
    ap.add_argument("--only-bench", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gdec_post_refactor.json"))
    args = ap.parse_args()
    if args.child:
        return child(args.frames, args.rounds, args.warm_rounds, args.n)
    libs = {"parent": os.path.join(REPO, "build", "variants", args.parent, "libhjd.so"), "branch": ""}
    runs = {name: [] for name in libs}
    for rep in range(args.reps):
        for name, lib in libs.items():   # alternating
            r = {} if args.only_bench else run_child(lib, args)
            if not args.skip_bench:
                r.update(run_bench(lib, args))
            runs[name].append(r)
            print(rep, name, json.dumps(r), file=sys.stderr, flush=True)
    numbers = {}
    for key in runs["parent"][0]:
        pv, bv = [r[key] for r in runs["parent"]], [r[key] for r in runs["branch"]]
        rate = key.endswith("Mpx_s")
        med = statistics.median(bv)
        numbers[key] = {"parent": [round(v, 4) for v in pv], "branch": [round(v, 4) for v in bv],
                        "parent_min": round(min(pv), 4), "parent_median": round(statistics.median(pv), 4),
                        "parent_max": round(max(pv), 4), "branch_median": round(med, 4),
                        "higher_is_better": rate,
                        "within": med >= min(pv) * 0.98 if rate else med <= max(pv) * 1.02}
    result = {"what": "parent library against the branch's, alternating child processes; criterion per number: the "
                      "branch's median within the parent's min..max over its repetitions widened by 2 %",
              "reps": args.reps, "frames": args.frames, "rounds": args.rounds, "warm_rounds": args.warm_rounds,
              "latency_calls": args.n, "bench_args": None if args.skip_bench else args.bench_args,
              "numbers": numbers, "all_within": all(v["within"] for v in numbers.values())}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"gdec_post_ab": "ok", "all_within": result["all_within"], "file": os.path.relpath(args.out, REPO)}))


if __name__ == "__main__":
    main()

"""A/B of the EXIF orientation on the GPU (backend.Orient and
GpuDecoder.decode_rgb_oriented()) against what it replaces,
one device, same run.

    python tools/orient_ab.py [--frames 256] [--rounds 10] [--out profiles/orient_ab.json]

(a) The kernel alone.  `frames` planar uint8 FHD frames (3 x 1080 x 1920 random
bytes each), the whole batch in orientation 3, then 6, then 8, uint8 out, one
launch; against a device-to-device copy of the same bytes (Tensor.copy_).  A
permutation is memory bound, so the copy is the yardstick; the figure is the
ratio of the medians, and the algorithmic bytes (read + written) over the
median as a fraction of 8 TB/s.  Device events around `--reps` back-to-back
launches; the legs alternate inside every round.  Before timing each leg's
output must equal torch's flip / rot90 of the frames byte for byte.  The same
legs are repeated on 1920 x 1024 frames, whose transposed rows (1024 bytes) are
a multiple of the 128-byte line where FHD's (1080) are not.

(b) End to end.  `frames` q90 4:2:0 FHD JPEGs (bench.py's synthetic files, a
pool of distinct ones cycled) of which every 8th carries EXIF orientation 6,
decoded to float16 with ImageNet mean / std:
  oriented    decode_rgb_oriented(apply_exif_orientation=True, dtype=float16, mean=, std=)
  torch       the route it replaces: decode_rgb() to uint8 planes, then per
              image rot90 / contiguous where tagged and the normalisation
              (addcmul in half) into new tensors
  all1        the same files with every tag 1 through apply_exif_orientation=True
  plain       those files through decode_rgb(dtype=float16, ...) without the
              argument: the code path the feature leaves untouched
Host clock around the call with a device synchronise before and inside the
window (the torch route is hundreds of small launches whose cost is on the
host); interleaved rounds after untimed warm rounds.  `unchanged_path`: all1's
median inside plain's own min .. max over the rounds.  Before timing, oriented
must equal the Orient kernel applied to the plain decode bit for bit and agree
with the torch route to 0.02 in normalised units.
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

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
W, H = 1920, 1080
POOL = 8
HBM_BYTES_PER_MS = 8e9   # 8 TB/s


def exif_segment(orientation: int) -> bytes:
    """An APP1 with a big-endian TIFF block whose IFD0 holds only the Orientation tag."""
    tiff = (b"MM\x00\x2a\x00\x00\x00\x08" + b"\x00\x01" + b"\x01\x12\x00\x03\x00\x00\x00\x01" +
            int(orientation).to_bytes(2, "big") + b"\x00\x00" + b"\x00\x00\x00\x00")
    payload = b"Exif\x00\x00" + tiff
    return b"\xff\xe1" + (len(payload) + 2).to_bytes(2, "big") + payload


def tagged(jpeg: bytes, orientation: int) -> bytes:
    assert jpeg[:2] == b"\xff\xd8"
    return jpeg[:2] + exif_segment(orientation) + jpeg[2:]


def stats(v):
    return {"ms_min": round(min(v), 4), "ms_median": round(statistics.median(v), 4), "ms_max": round(max(v), 4),
            "ms_rounds": [round(t, 4) for t in v]}


def torch_orient(torch, x, o):
    """What the kernel computes for o in (3, 6, 8), by torch, on (..., h, w)."""
    if o == 3:
        return x.flip(-1).flip(-2)
    return torch.rot90(x, k=-1 if o == 6 else 1, dims=(-2, -1))


def kernel_alone(torch, hjd, ctx, dev, nf, rounds, warm_rounds, reps, W=W, H=H):
    gen = torch.Generator(device=dev).manual_seed(5)
    src = torch.randint(0, 256, (nf, 3, H, W), dtype=torch.uint8, device=dev, generator=gen)
    copy_dst = torch.empty_like(src)
    stream = torch.cuda.current_stream()
    legs, keep = {"copy": lambda: copy_dst.copy_(src)}, []
    for o in (3, 6, 8):
        shape = (nf, 3, W, H) if o >= 5 else (nf, 3, H, W)
        out = torch.zeros(shape, dtype=torch.uint8, device=dev)
        op = hjd.Orient(ctx, [src[i] for i in range(nf)], [out[i] for i in range(nf)], [o] * nf)
        op.launch(stream)
        torch.cuda.synchronize()
        if not torch.equal(out, torch_orient(torch, src, o)):
            raise SystemExit(f"orientation {o}: the kernel differs from torch's flip / rot90")
        keep.append((op, out))
        legs[f"orient_{o}"] = (lambda op=op: op.launch(stream))

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
    nbytes = 2 * src.numel()
    res = {"frames": nf, "width": W, "height": H, "dtype": "uint8", "launches_per_sample": reps,
           "algorithmic_bytes": nbytes, "timing": "device events around the back-to-back launches, per launch",
           "legs": {name: stats(v) for name, v in ms.items()}}
    copy_med = res["legs"]["copy"]["ms_median"]
    for name, leg in res["legs"].items():
        leg["fraction_of_8TBps"] = round(nbytes / leg["ms_median"] / HBM_BYTES_PER_MS, 4)
        leg["vs_copy"] = round(leg["ms_median"] / copy_med, 4)
    for op, _ in keep:
        op.close()
    del keep, src, copy_dst
    torch.cuda.empty_cache()
    return res


def end_to_end(torch, hjd, ctx, dev, nf, rounds, warm_rounds):
    import bench
    pool = bench.encode_pool(W, H, hjd.YUV420, min(POOL, nf), seed0=9300)
    base = [pool[i % len(pool)] for i in range(nf)]
    orients = [6 if i % 8 == 7 else 1 for i in range(nf)]
    mixed = [tagged(d, o) for d, o in zip(base, orients)]
    all1 = [tagged(d, 1) for d in base]
    if [hjd.exif_orientation(d) for d in mixed] != orients or any(hjd.exif_orientation(d) != 1 for d in all1):
        raise SystemExit("the tags written are not the tags read")
    info = hjd.parse(base[0])
    a_np, b_np = hjd.norm_constants(MEAN, STD)
    a16 = torch.tensor(a_np, device=dev).view(3, 1, 1).half()
    b16 = torch.tensor(b_np, device=dev).view(3, 1, 1).half()
    gd = hjd.GpuDecoder(ctx, nf, 2 * sum(map(len, mixed)), nf * info.nblocks)
    kw = dict(dtype=torch.float16, mean=MEAN, std=STD)
    last = {}

    def leg_oriented():
        last["oriented"] = gd.decode_rgb_oriented(mixed, apply_exif_orientation=True, **kw)
        gd.sync()

    def leg_torch():
        planes = gd.decode_rgb(mixed)
        gd.sync()
        outs = []
        for p, o in zip(planes, orients):
            if o == 6:
                p = torch.rot90(p, k=-1, dims=(1, 2)).contiguous()
            outs.append(torch.addcmul(b16, p.half(), a16))
        last["torch"] = outs

    def leg_all1():
        last["all1"] = gd.decode_rgb_oriented(all1, apply_exif_orientation=True, **kw)
        gd.sync()

    def leg_plain():
        last["plain"] = gd.decode_rgb(all1, **kw)
        gd.sync()

    jobs = [("oriented", leg_oriented), ("torch", leg_torch), ("all1", leg_all1), ("plain", leg_plain)]
    for _ in range(max(1, warm_rounds)):
        for _, job in jobs:
            job()
    torch.cuda.synchronize()
    # oriented == Orient(plain uint8 decode) bit for bit; ~ the torch route; all1 == plain
    planes = gd.decode_rgb(mixed)
    gd.sync()
    outs = [torch.zeros((3, W, H) if o == 6 else (3, H, W), dtype=torch.float16, device=dev) for o in orients]
    op = hjd.Orient(ctx, planes, outs, orients, normalize=(a_np, b_np))
    op.launch(torch.cuda.current_stream())
    torch.cuda.synchronize()
    op.close()
    agree = 0.0
    for i in range(nf):
        if not torch.equal(outs[i].view(torch.int16), last["oriented"][i].view(torch.int16)):
            raise SystemExit(f"image {i}: the oriented decode differs from the Orient kernel on the plain decode")
        if not torch.equal(last["all1"][i].view(torch.int16), last["plain"][i].view(torch.int16)):
            raise SystemExit(f"image {i}: the all-1 oriented decode differs from the plain decode")
        agree = max(agree, float((last["torch"][i].float() - last["oriented"][i].float()).abs().max()))
    if agree > 0.02:
        raise SystemExit(f"the oriented decode and the torch route differ by {agree} in normalised units")
    del outs, planes

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
    res = {"frames": nf, "width": W, "height": H, "distinct_files": len(pool), "tagged_6": sum(o == 6 for o in orients),
           "jpeg_bytes": sum(map(len, mixed)), "dtype": "float16", "max_abs_diff_torch_vs_oriented": agree,
           "timing": "host clock around the call, a device synchronise before and inside the window",
           "legs": {name: stats(v) for name, v in ms.items()}}
    L = res["legs"]
    res["holds"] = {"oriented_vs_torch": round(L["oriented"]["ms_median"] / L["torch"]["ms_median"], 4),
                    "oriented_below_torch": L["oriented"]["ms_median"] < L["torch"]["ms_median"],
                    "oriented_vs_plain": round(L["oriented"]["ms_median"] / L["plain"]["ms_median"], 4),
                    "all1_vs_plain": round(L["all1"]["ms_median"] / L["plain"]["ms_median"], 4),
                    "unchanged_path": L["plain"]["ms_min"] <= L["all1"]["ms_median"] <= L["plain"]["ms_max"]}
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "orient_ab.json"))
    args = ap.parse_args()
    import torch
    import ocljpegdecoder_amd as hjd
    if not torch.cuda.is_available():
        raise SystemExit("orient_ab needs a GPU: no timing is taken without one")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = hjd.Context(0)
    result = {"tool": "tools/orient_ab.py", "utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
              "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "frames": args.frames,
              "rounds": args.rounds, "warm_rounds": args.warm_rounds, "mean": list(MEAN), "std": list(STD),
              "method": "untimed interleaved warm rounds of every leg, then interleaved rounds; medians with min and max"}
    result["kernel_alone"] = kernel_alone(torch, hjd, ctx, dev, args.frames, args.rounds, args.warm_rounds, args.reps)
    for name, leg in result["kernel_alone"]["legs"].items():
        print(f"kernel {name:10s} {leg['ms_median']:9.4f} ms (median) {leg['ms_max']:9.4f} (max) "
              f"x{leg['vs_copy']} of the copy, {leg['fraction_of_8TBps']} of 8 TB/s", file=sys.stderr, flush=True)
    # the same with 1024 rows: the transposed outputs' pitch (1024 against 1080) is then a multiple of the
    # 128-byte line, which separates what the pitch costs orientations 6 and 8 from what the exchange costs
    result["kernel_alone_1920x1024"] = kernel_alone(torch, hjd, ctx, dev, args.frames, args.rounds, args.warm_rounds,
                                                    args.reps, W=1920, H=1024)
    for name, leg in result["kernel_alone_1920x1024"]["legs"].items():
        print(f"kernel/1024 {name:10s} {leg['ms_median']:9.4f} ms (median) x{leg['vs_copy']} of the copy",
              file=sys.stderr, flush=True)
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
    print(json.dumps({"orient_ab": "ok", "file": os.path.relpath(args.out, REPO)}))


if __name__ == "__main__":
    main()

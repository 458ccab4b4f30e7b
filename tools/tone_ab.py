"""A/B of the tone stage on the GPU (backend.Tone and
GpuDecoder.decode_rgb_resized_tone()) against the route it replaces, one
device, same run.

    python tools/tone_ab.py [--frames 256] [--rounds 10] [--out profiles/tone_ab.json]
    python tools/tone_ab.py --probe      # one launch of each Tone object of (a): for a counter collection

First, on a small case (three sources of different sizes, the three modes),
Tone's output must equal the numpy model's (tests/tone_model.py) bit for bit.

(a) The kernels alone.  `frames` x 3 x 224 x 224 random bytes to float16 with
ImageNet constants:
  tone_table         Tone, all TONE_TABLE with a solarize table: one launch
  tone_autocontrast  Tone, all TONE_AUTOCONTRAST: the histogram, curve and tone launches
  tone_equalize      Tone, all TONE_EQUALIZE: the same three
  color_m            Color with records whose p is 0: one launch that moves the same bytes
  copy_u8            a device copy of the bytes read (Tensor.copy_)
  copy_f16           a device copy of the bytes written
Device events around `--reps` back-to-back launches; the legs alternate inside
every round; medians with min and max.

(b) End to end.  `frames` q90 4:2:0 FHD JPEGs (bench.py's synthetic files, a
pool of distinct ones cycled), each with its own random-resized crop (8 % ..
100 % of the area, aspect 3/4 .. 4/3) and flip, every second one equalized
and the others solarized at 128, to 224 x 224 float16 with ImageNet mean /
std:
  tone     decode_rgb_resized_tone(size, rois=, flips=, curves=, modes=, dtype=float16, mean=, std=)
  resized  decode_rgb_resized(...) of the same crops to float16 without tones: what the stage adds to
  torch    the route it replaces: decode_rgb_resized() to uint8, then in torch
           one bincount over (image, channel, value), cumsum, the integer
           curve of include/hjd.h, a gather and the normalisation, rounded to
           half
Host clock around the call with a device synchronise before and inside the
window; interleaved rounds after untimed warm rounds.  Before timing, the
bytes of `tone` (a uint8 call) and of the torch route must be equal -- both are
exact integer statements of the same map -- and the float16 results within
2^-9 of each other (an fma against a multiply and an add, each rounded to
half).
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
    """Tone against tests/tone_model.py on a small case, bit for bit."""
    import tone_model
    shapes = [(37, 29), (300, 200), (5, 3)]
    modes = [hjd.TONE_EQUALIZE, hjd.TONE_AUTOCONTRAST, hjd.TONE_TABLE]
    curves = [hjd.tone_curve(solarize=128), hjd.tone_curve(gamma=0.7), hjd.tone_curve(posterize=3)]
    a, b = hjd.norm_constants(MEAN, STD)
    rng = np.random.default_rng(7)
    host = [rng.integers(20, 220, (3, h, w), dtype=np.uint8) for w, h in shapes]
    srcs = [torch.from_numpy(s).to(dev) for s in host]
    outs = [torch.zeros(s.shape, dtype=torch.float16, device=dev) for s in host]
    op = hjd.Tone(ctx, srcs, outs, curves=curves, modes=modes, normalize=(a, b))
    op.launch(torch.cuda.current_stream())
    torch.cuda.synchronize()
    op.close()
    for k in range(3):
        exp = tone_model.tone(host[k], modes[k], curves[k], np.float16, tuple(float(v) for v in a), tuple(float(v) for v in b))
        if not np.array_equal(outs[k].cpu().numpy().view(np.uint16), exp):
            raise SystemExit(f"item {k}: Tone differs from the model")


def kernel_alone(torch, hjd, ctx, dev, nf, rounds, warm_rounds, reps, probe=False):
    gen = torch.Generator(device=dev).manual_seed(5)
    src = torch.randint(0, 256, (nf, 3, OUT, OUT), dtype=torch.uint8, device=dev, generator=gen)
    srcs = [src[i] for i in range(nf)]
    norm = hjd.norm_constants(MEAN, STD)
    stream = torch.cuda.current_stream()
    outs = {name: torch.zeros((nf, 3, OUT, OUT), dtype=torch.float16, device=dev)
            for name in ("tone_table", "tone_autocontrast", "tone_equalize", "color_m")}
    copy_u8, copy_f16 = torch.empty_like(src), torch.empty_like(outs["color_m"])
    ops = {"tone_table": hjd.Tone(ctx, srcs, outs["tone_table"], curves=hjd.tone_curve(solarize=128), normalize=norm),
           "tone_autocontrast": hjd.Tone(ctx, srcs, outs["tone_autocontrast"], modes=hjd.TONE_AUTOCONTRAST, normalize=norm),
           "tone_equalize": hjd.Tone(ctx, srcs, outs["tone_equalize"], modes=hjd.TONE_EQUALIZE, normalize=norm),
           "color_m": hjd.Color(ctx, srcs, outs["color_m"], [hjd.color_matrix(brightness=1.2, saturation=0.8)] * nf,
                                normalize=norm)}
    if probe:
        for op in ops.values():
            op.launch(stream)
        torch.cuda.synchronize()
        for op in ops.values():
            op.close()
        return {"frames": nf, "launched_once": list(ops)}
    legs = {"copy_u8": lambda: copy_u8.copy_(src), "copy_f16": lambda: copy_f16.copy_(outs["color_m"])}
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
    res = {"frames": nf, "size": [OUT, OUT], "dtype": "float16", "launches_per_sample": reps,
           "bytes_read": src.numel(), "bytes_written": copy_f16.numel() * 2,
           "timing": "device events around the back-to-back launches, per launch",
           "legs": {name: stats(v) for name, v in ms.items()}}
    L = res["legs"]
    for leg in L.values():
        leg["vs_copy_f16"] = round(leg["ms_median"] / L["copy_f16"]["ms_median"], 4)
    res["holds"] = {"tone_table_vs_color_m": round(L["tone_table"]["ms_median"] / L["color_m"]["ms_median"], 4),
                    "tone_equalize_vs_tone_table": round(L["tone_equalize"]["ms_median"] / L["tone_table"]["ms_median"], 4)}
    for op in ops.values():
        op.close()
    del src, srcs, outs, copy_u8, copy_f16
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


def torch_tone(torch, u8, equalize, table):
    """The bytes of the tone stage on a (n, 3, h, w) uint8 batch, in torch: image i through equalize
    (equalize[i]) or through `table` (256 values).  The integer curve of include/hjd.h."""
    n, _, h, w = u8.shape
    dev = u8.device
    idx = u8.long() + (torch.arange(n * 3, device=dev) * 256).view(n, 3, 1, 1)
    hist = torch.bincount(idx.flatten(), minlength=n * 3 * 256).view(n, 3, 256)
    full = hist > 0
    lo = full.int().argmax(-1)
    hi = 255 - full.flip(-1).int().argmax(-1)
    last = hist.gather(-1, hi.unsqueeze(-1)).squeeze(-1)
    step = (h * w - last) // 255
    below = hist.cumsum(-1) - hist
    v = torch.arange(256, device=dev)
    curve = torch.clamp(((step // 2).unsqueeze(-1) + below) // step.clamp(min=1).unsqueeze(-1), max=255)
    curve = torch.where(((hi == lo) | (step == 0)).unsqueeze(-1), v, curve)
    lut = torch.where(equalize.view(n, 1, 1), curve, table.view(1, 1, 256))
    return lut.flatten()[idx].to(torch.uint8)


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
    sol = hjd.tone_curve(solarize=128)
    modes = [hjd.TONE_EQUALIZE if i % 2 == 0 else hjd.TONE_TABLE for i in range(nf)]
    curves = [hjd.TONE_IDENTITY if i % 2 == 0 else sol for i in range(nf)]
    equalize = torch.tensor([m == hjd.TONE_EQUALIZE for m in modes], device=dev)
    table = torch.from_numpy(sol[0].astype(np.int64)).to(dev)
    a_np, b_np = hjd.norm_constants(MEAN, STD)
    a32 = torch.tensor(a_np, device=dev).view(1, 3, 1, 1)
    b32 = torch.tensor(b_np, device=dev).view(1, 3, 1, 1)

    def leg_resized():
        last["resized"] = gd.decode_rgb_resized(datas, (OUT, OUT), flips=flips, rois=rois, dtype=torch.float16,
                                                mean=MEAN, std=STD)
        gd.sync()

    def leg_tone():
        last["tone"] = gd.decode_rgb_resized_tone(datas, (OUT, OUT), flips=flips, rois=rois, curves=curves, modes=modes,
                                                  dtype=torch.float16, mean=MEAN, std=STD)
        gd.sync()

    def leg_torch():
        u8 = gd.decode_rgb_resized(datas, (OUT, OUT), flips=flips, rois=rois)
        gd.sync()
        last["torch_u8"] = torch_tone(torch, u8, equalize, table)
        last["torch"] = torch.addcmul(b32, last["torch_u8"].float(), a32).half()

    jobs = [("resized", leg_resized), ("tone", leg_tone), ("torch", leg_torch)]
    for _ in range(max(1, warm_rounds)):
        for _, job in jobs:
            job()
    torch.cuda.synchronize()
    tone_u8 = gd.decode_rgb_resized_tone(datas, (OUT, OUT), flips=flips, rois=rois, curves=curves, modes=modes)
    gd.sync()
    if not torch.equal(tone_u8, last["torch_u8"]):
        raise SystemExit("the tone decode and the torch route give different bytes")
    diff = float((last["tone"].float() - last["torch"].float()).abs().max())
    if diff > 2.0 ** -9:   # |values| < 4: one step of half precision there
        raise SystemExit(f"the float16 results differ by {diff}")
    res = {"frames": nf, "width": W, "height": H, "out": [OUT, OUT], "distinct_files": len(pool),
           "jpeg_bytes": sum(map(len, datas)), "dtype": "float16", "crop_area": [0.08, 1.0],
           "decoded_pixel_fraction": round(sum(r[2] * r[3] for r in rois) / (nf * W * H), 4),
           "tones": "even images equalized (TONE_EQUALIZE, identity table), odd ones solarized at 128 (TONE_TABLE)",
           "bytes_equal_torch_route": True, "max_abs_diff_float16": diff,
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
    res["holds"] = {"tone_vs_torch": round(L["tone"]["ms_median"] / L["torch"]["ms_median"], 4),
                    "tone_minus_resized_ms": round(L["tone"]["ms_median"] - L["resized"]["ms_median"], 4),
                    "tone_below_torch": L["tone"]["ms_median"] < L["torch"]["ms_median"]}
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
                    help="launch each object of (a) once and stop: the run a counter collection wraps")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tone_ab.json"))
    args = ap.parse_args()
    import torch
    import ocljpegdecoder_amd as hjd
    if not torch.cuda.is_available():
        raise SystemExit("tone_ab needs a GPU: no timing is taken without one")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = hjd.Context(0)
    if args.probe:
        print(json.dumps({"tone_ab": "probe", **kernel_alone(torch, hjd, ctx, dev, args.frames, 0, 0, 1, probe=True)}))
        ctx.close()
        return
    result = {"tool": "tools/tone_ab.py", "utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
              "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "frames": args.frames,
              "rounds": args.rounds, "warm_rounds": args.warm_rounds, "mean": list(MEAN), "std": list(STD),
              "method": "untimed interleaved warm rounds of every leg, then interleaved rounds; medians with min and max"}
    model_check(torch, hjd, ctx, dev)
    result["model_check"] = "Tone == tests/tone_model.py on 3 items of different sizes, the three modes, float16"
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
    print(json.dumps({"tone_ab": "ok", "file": os.path.relpath(args.out, REPO)}))


if __name__ == "__main__":
    main()

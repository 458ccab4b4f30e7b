"""A/B of the scaled decode (1/2, 1/4, 1/8) against the full-size decode, one
device, same run.

    python tools/scaled_decode_ab.py [--frames 256] [--rounds 12] [--out profiles/scaled_decode_ab.json]

Persistent kernel, 3840x2160 frames, 4:2:0 and 4:4:4, int16 zigzag input,
OUT_RGB_PLANAR and OUT_BGRX, scale 1, 2, 4, 8.  All legs of a sampling decode
the same coefficient buffer; after untimed interleaved warm rounds of every leg
they are timed with device events in interleaved rounds (one launch of each leg
per round), so drift hits all alike.  Before any number is reported each
scale's BGRX output is checked against its planar output, permuted.

Per leg: ms per launch (minimum and median over the rounds), source Mpx/s, the
algorithmic bytes per source pixel (coefficient bytes + output bytes, from the
shapes) and `spread`, (max - min) / min over the rounds.  `two_pass` is today's
route to a small planar tensor, timed as a whole: the full-size planar decode
followed by torch.nn.functional.avg_pool2d(x.float(), s).  `holds` records the
checks: every scaled leg's median against the same run's scale-1 median plus
that leg's max - min, and against the two-pass route.

`fhd_gpu_decoder`: one FHD q90 4:2:0 JPEG through GpuDecoder.decode_rgb at
scale 1 and 4, wall-clock ms per image (the scaled decode has no latency
kernel; this is what that costs).
"""
from __future__ import annotations

import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from out_format_ab import H, W, POOL, qtables, synth_frame   # noqa: E402  (the same synthetic frames)

SCALES = (1, 2, 4, 8)


def run_sampling(torch, hjd, ctx, dev, sampling, nf, rounds, warm_rounds):
    qt = qtables()
    mw, mh, bpm, _ = hjd.mcu_geometry(W, H, sampling)
    nblk = mw * mh * bpm
    coefs = torch.empty((nf, nblk, 64), dtype=torch.int16, device=dev)
    for i in range(min(POOL, nf)):
        coefs[i] = synth_frame(torch, hjd, nblk, sampling, qt, seed=7000 + i, dev=dev)
    for i in range(POOL, nf):
        coefs[i].copy_(coefs[i % POOL])
    formats = [("rgb_planar", hjd.OUT_RGB_PLANAR), ("bgrx", hjd.OUT_BGRX)]
    legs, plans, outs, shape = [], {}, {}, {}
    for s in SCALES:
        sw, sh = hjd.scaled_size(W, H, s)
        shape[s] = (sw, sh)
        for name, fmt in formats:
            pitch = hjd.default_pitch(sw, fmt)
            frame_bytes = pitch * hjd.backend.out_rows(sh, fmt)
            key = (name, s)
            legs.append(key)
            outs[key] = torch.zeros((nf, frame_bytes), dtype=torch.uint8, device=dev)
            specs = [hjd.FrameSpec(W, H, sampling, coef_offset=i * nblk, out_offset=i * frame_bytes, out_pitch=pitch,
                                   qt_index=(0, 1, 2), out_format=fmt) for i in range(nf)]
            plans[key] = hjd.Plan(ctx, specs, hjd.IN_Q16_ZIGZAG, qtables=qt, scale=s)
            plans[key].set_kernel(hjd.KERNEL_PERSISTENT)
    stream = torch.cuda.current_stream()

    def two_pass(s):
        plans[("rgb_planar", 1)].launch(coefs, outs[("rgb_planar", 1)], stream)
        x = outs[("rgb_planar", 1)].view(nf, 3, H, W)
        return torch.nn.functional.avg_pool2d(x.float(), s)

    def consistent():
        for s in SCALES:
            sw, sh = shape[s]
            k = min(nf, 16)
            b = outs[("bgrx", s)][:k].view(k, sh, sw, 4)
            p = outs[("rgb_planar", s)][:k].view(k, 3, sh, sw)
            if not torch.equal(p, b[..., [2, 1, 0]].permute(0, 3, 1, 2)):
                raise SystemExit(f"scale {s}: the planar and BGRX outputs of this run differ")

    for _ in range(max(1, warm_rounds)):   # warm launches of each leg, interleaved like the timed ones
        for key in legs:
            plans[key].launch(coefs, outs[key], stream)
        for s in SCALES[1:]:
            del_me = two_pass(s)
            del del_me
    torch.cuda.synchronize()
    consistent()
    ms = {key: [] for key in legs}
    ms2 = {s: [] for s in SCALES[1:]}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        r = fn()
        e1.record(stream)
        e1.synchronize()
        del r
        return e0.elapsed_time(e1)

    for _ in range(rounds):
        for key in legs:
            ms[key].append(timed(lambda: plans[key].launch(coefs, outs[key], stream)))
        for s in SCALES[1:]:
            ms2[s].append(timed(lambda: two_pass(s)))
    consistent()
    px = nf * W * H
    res = {"legs": {}, "two_pass": {}, "holds": {}}
    for name, fmt in formats:
        for s in SCALES:
            v = ms[(name, s)]
            sw, sh = shape[s]
            nbytes = plans[(name, s)].coef_bytes + nf * sw * sh * hjd.OUT_BYTES[fmt]
            res["legs"][f"{name}_s{s}"] = {
                "scale": s, "out_format": name, "out_size": [sw, sh],
                "ms_min": round(min(v), 4), "ms_median": round(statistics.median(v), 4), "ms_max": round(max(v), 4),
                "ms_rounds": [round(x, 4) for x in v], "spread": round((max(v) - min(v)) / min(v), 4),
                "source_mpx_per_s": round(px / min(v) / 1e3, 1),
                "source_mpx_per_s_median": round(px / statistics.median(v) / 1e3, 1),
                "algorithmic_bytes": int(nbytes), "bytes_per_source_px": round(nbytes / px, 3),
                "launch_shape": plans[(name, s)].launch_shape()}
    for s in SCALES[1:]:
        v = ms2[s]
        res["two_pass"][f"s{s}"] = {"route": "full-size planar decode + avg_pool2d(x.float(), s)",
                                    "ms_min": round(min(v), 4), "ms_median": round(statistics.median(v), 4),
                                    "ms_rounds": [round(x, 4) for x in v]}
    for name, _ in formats:
        one = res["legs"][f"{name}_s1"]
        slack = one["ms_max"] - one["ms_min"]   # the round-to-round spread of the scale-1 leg, in ms
        for s in SCALES[1:]:
            leg = res["legs"][f"{name}_s{s}"]
            res["holds"][f"{name}_s{s}"] = {
                "median_vs_s1": round(leg["ms_median"] / one["ms_median"], 4),
                "no_slower_than_s1_plus_spread": leg["ms_median"] <= one["ms_median"] + slack,
                "s1_spread_ms": round(slack, 4),
                "speedup_over_two_pass": round(res["two_pass"][f"s{s}"]["ms_median"] / leg["ms_median"], 3),
                "faster_than_two_pass": leg["ms_median"] < res["two_pass"][f"s{s}"]["ms_median"]}
    for p in plans.values():
        p.close()
    del coefs, outs
    torch.cuda.empty_cache()
    return res


def fhd_gpu_decoder(torch, hjd, ctx, iters=40):
    """One FHD q90 4:2:0 JPEG through GpuDecoder.decode_rgb, wall-clock ms per image."""
    from PIL import Image
    rng = np.random.default_rng(11)
    w, h = 1920, 1080
    x = np.linspace(0, 255, w)[None, :, None]
    y = np.linspace(0, 255, h)[:, None, None]
    img = np.clip(x * [1, 0, 0.5] + y * [0, 1, 0.5] + rng.normal(0, 20, (h, w, 3)), 0, 255).astype(np.uint8)
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="JPEG", quality=90, subsampling=2)
    data = b.getvalue()
    info = hjd.parse(data)
    res = {"width": w, "height": h, "quality": 90, "jpeg_bytes": len(data), "iters": iters}
    with hjd.GpuDecoder(ctx, 1, 2 * len(data), info.nblocks) as gd:
        for s in (1, 4):
            sw, sh = hjd.scaled_size(w, h, s)
            out = torch.empty((1, 3, sh, sw), dtype=torch.uint8, device="cuda")
            t = []
            for i in range(iters + 5):
                t0 = time.perf_counter()
                gd.decode_rgb([data], out=out, scale=s)
                gd.sync()
                if i >= 5:
                    t.append((time.perf_counter() - t0) * 1e3)
            res[f"scale_{s}"] = {"ms_per_image_median": round(statistics.median(t), 4), "ms_per_image_min": round(min(t), 4),
                                 "pixel_kernel": "latency (AUTO)" if s == 1 else "persistent (the scaled decode has no latency kernel)"}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warm-rounds", type=int, default=3, help="untimed interleaved rounds before the timed ones")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "scaled_decode_ab.json"))
    args = ap.parse_args()
    import torch
    import ocljpegdecoder_amd as hjd
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = hjd.Context(0)
    result = {"tool": "tools/scaled_decode_ab.py", "utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
              "device": torch.cuda.get_device_name(0), "width": W, "height": H, "frames": args.frames,
              "rounds": args.rounds, "warm_rounds": args.warm_rounds, "input": "int16 zigzag",
              "kernel": "persistent, shape-default launch",
              "method": "untimed interleaved warm rounds of every leg, then interleaved rounds of one event-timed "
                        "launch per leg (the two-pass routes in the same rounds); each scale's BGRX output checked "
                        "against its planar output before and after timing",
              "d16_gather": list(ctx.d16_gather()), "samplings": {}}
    for sname, s in (("4:2:0", hjd.YUV420), ("4:4:4", hjd.YUV444)):
        r = run_sampling(torch, hjd, ctx, dev, s, args.frames, args.rounds, args.warm_rounds)
        result["samplings"][sname] = r
        for name, leg in r["legs"].items():
            print(f"{sname} {name:14s} {leg['ms_median']:8.3f} ms (median)  {leg['source_mpx_per_s_median']:10.1f} "
                  f"source Mpx/s  {leg['bytes_per_source_px']:.3f} B/px  spread {leg['spread']:.3f}",
                  file=sys.stderr, flush=True)
        for name, tp in r["two_pass"].items():
            print(f"{sname} two-pass {name:5s} {tp['ms_median']:8.3f} ms (median)", file=sys.stderr, flush=True)
    result["fhd_gpu_decoder"] = fhd_gpu_decoder(torch, hjd, ctx)
    print("fhd", json.dumps(result["fhd_gpu_decoder"]), file=sys.stderr, flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"scaled_decode_ab": "ok", "file": os.path.relpath(args.out, REPO)}))


if __name__ == "__main__":
    main()

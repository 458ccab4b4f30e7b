"""A/B of the region-of-interest decode against the whole-frame decode, one
device, same run.

    python tools/roi_decode_ab.py [--frames 256] [--rounds 12] [--out profiles/roi_decode_ab.json]

Persistent kernel, 3840x2160 frames, 4:2:0 and 4:4:4, int16 zigzag input,
OUT_RGB_PLANAR and OUT_BGRX.  All legs of a sampling decode the same
coefficient buffer; after untimed interleaved warm rounds of every leg they
are timed with device events in interleaved rounds (one launch of each leg per
round), so drift hits all alike.  Before and after timing every ROI leg's
output is checked against the slice of the whole-frame leg's output.

Legs (per sampling and output format):
  a        the plan without ROIs
  b        a ROI equal to the whole frame (the ROI kernels' full path)
  a2       control: leg a again, into an output allocation of its own (what a
           different allocation alone does to the time)
  b_in_a   control: leg b writing into leg a's output allocation
  c        a centred 1920x1080 ROI, x % 4 == 0 (vector stores in interior strips)
  d        the same rectangle shifted to an odd x (guarded byte stores everywhere)
  e        a centred 224x224 ROI
  f_c, f_e the source regions of c and e at scale 2 (960x540 and 112x112 on the
           1920x1080 grid)
  g_c, g_e the route a ROI replaces: leg a followed by
           out[..., y:y+h, x:x+w].contiguous() for the c and e rectangles

Per leg: ms per launch (minimum, median and maximum over the rounds, and
`spread` = (max - min) / min), the plan's tasks, and the algorithmic bytes
(coefficient bytes the tasks read plus bytes written).  `holds` records the one
pass/fail comparison: leg b's median must lie within leg a's own round-to-round
spread of the same run (b_median <= a_max); the other legs are reported beside
their task counts (ms per task relative to leg a) and against g.

`fhd_gpu_decoder`: one FHD q90 4:2:0 JPEG through GpuDecoder.decode_rgb
without a ROI (the latency kernel), with the whole-frame ROI and with a centred
224x224 ROI (a ROI launch has no latency kernel), wall-clock ms per image.
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

RECT_C = (960, 540, 1920, 1080)
RECT_D = (961, 540, 1920, 1080)
RECT_E = (1808, 968, 224, 224)
# (name, scale, roi)
LEGS = [("a", 1, None), ("b", 1, (0, 0, W, H)), ("a2", 1, None), ("b_in_a", 1, (0, 0, W, H)),
        ("c", 1, RECT_C), ("d", 1, RECT_D), ("e", 1, RECT_E),
        ("f_c", 2, tuple(v // 2 for v in RECT_C)), ("f_e", 2, tuple(v // 2 for v in RECT_E))]


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
    keys, plans, outs, size = [], {}, {}, {}
    for fname, fmt in formats:
        for leg, scale, roi in LEGS:
            spec0 = hjd.FrameSpec(W, H, sampling, out_format=fmt, roi=roi)
            ow, oh = spec0.out_size(scale)
            pitch = hjd.default_pitch(ow, fmt)
            frame_bytes = pitch * hjd.backend.out_rows(oh, fmt)
            key = (fname, leg)
            keys.append(key)
            size[key] = (ow, oh)
            outs[key] = (outs[(fname, "a")] if leg == "b_in_a" else
                         torch.zeros((nf, frame_bytes), dtype=torch.uint8, device=dev))
            specs = [hjd.FrameSpec(W, H, sampling, coef_offset=i * nblk, out_offset=i * frame_bytes, out_pitch=pitch,
                                   qt_index=(0, 1, 2), out_format=fmt, roi=roi) for i in range(nf)]
            plans[key] = hjd.Plan(ctx, specs, hjd.IN_Q16_ZIGZAG, qtables=qt, scale=scale)
            plans[key].set_kernel(hjd.KERNEL_PERSISTENT)
            assert plans[key].has_roi == (roi is not None)
    stream = torch.cuda.current_stream()

    def view(fname, key):
        ow, oh = size[key]
        return outs[key].view(nf, 3, oh, ow) if fname == "rgb_planar" else outs[key].view(nf, oh, ow, 4)

    def crop(fname, full, roi):
        x, y, w, h = roi
        return full[..., y:y + h, x:x + w] if fname == "rgb_planar" else full[:, y:y + h, x:x + w, :]

    def two_pass(fname, roi):
        plans[(fname, "a")].launch(coefs, outs[(fname, "a")], stream)
        return crop(fname, view(fname, (fname, "a")), roi).contiguous()

    def consistent():
        for fname, _ in formats:
            full = view(fname, (fname, "a"))
            for leg, scale, roi in LEGS:
                if roi is None or scale != 1 or leg == "b_in_a":
                    continue
                if not torch.equal(view(fname, (fname, leg)), crop(fname, full, roi)):
                    raise SystemExit(f"{fname} leg {leg}: the ROI output differs from the slice of the whole-frame output")
            # scale 2: the small ROI against the slice of the large one (both ROI plans of the same grid)
            c2, e2 = dict((l, r) for l, _, r in LEGS)["f_c"], dict((l, r) for l, _, r in LEGS)["f_e"]
            rel = (e2[0] - c2[0], e2[1] - c2[1], e2[2], e2[3])
            if not torch.equal(view(fname, (fname, "f_e")), crop(fname, view(fname, (fname, "f_c")), rel)):
                raise SystemExit(f"{fname}: the scale-2 ROI outputs disagree")

    g_legs = [("g_c", RECT_C), ("g_e", RECT_E)]
    for _ in range(max(1, warm_rounds)):   # warm launches of each leg, interleaved like the timed ones
        for key in keys:
            plans[key].launch(coefs, outs[key], stream)
        for fname, _ in formats:
            for _, roi in g_legs:
                del_me = two_pass(fname, roi)
                del del_me
    torch.cuda.synchronize()
    consistent()
    ms = {key: [] for key in keys}
    ms2 = {(fname, g): [] for fname, _ in formats for g, _ in g_legs}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        r = fn()
        e1.record(stream)
        e1.synchronize()
        del r
        return e0.elapsed_time(e1)

    for _ in range(rounds):
        for key in keys:
            ms[key].append(timed(lambda: plans[key].launch(coefs, outs[key], stream)))
        for fname, _ in formats:
            for g, roi in g_legs:
                ms2[(fname, g)].append(timed(lambda: two_pass(fname, roi)))
    consistent()
    res = {"legs": {}, "holds": {}, "per_task": {}}

    def stats(v):
        return {"ms_min": round(min(v), 4), "ms_median": round(statistics.median(v), 4), "ms_max": round(max(v), 4),
                "ms_rounds": [round(x, 4) for x in v], "spread": round((max(v) - min(v)) / min(v), 4)}

    for fname, fmt in formats:
        for leg, scale, roi in LEGS:
            key = (fname, leg)
            ow, oh = size[key]
            written = nf * ow * oh * hjd.OUT_BYTES[fmt]
            d = {"scale": scale, "roi": list(roi) if roi else None, "out_format": fname, "out_size": [ow, oh]}
            d.update(stats(ms[key]))
            d.update({"tasks": plans[key].tasks, "coef_bytes": plans[key].coef_bytes, "bytes_written": written,
                      "algorithmic_bytes": plans[key].coef_bytes + written, "launch_shape": plans[key].launch_shape()})
            res["legs"][f"{fname}_{leg}"] = d
        a = res["legs"][f"{fname}_a"]
        for g, roi in g_legs:
            d = {"route": "leg a + out[..., y:y+h, x:x+w].contiguous()", "roi": list(roi), "out_format": fname}
            d.update(stats(ms2[(fname, g)]))
            d.update({"tasks": a["tasks"], "algorithmic_bytes": a["algorithmic_bytes"] +
                      2 * nf * roi[2] * roi[3] * hjd.OUT_BYTES[fmt]})
            res["legs"][f"{fname}_{g}"] = d
        b = res["legs"][f"{fname}_b"]
        res["holds"][fname] = {
            "a_ms_min": a["ms_min"], "a_ms_median": a["ms_median"], "a_ms_max": a["ms_max"], "b_ms_median": b["ms_median"],
            "b_median_vs_a_median": round(b["ms_median"] / a["ms_median"], 4),
            "b_within_a_spread": b["ms_median"] <= a["ms_max"],
            "control_a2_median_vs_a_median": round(res["legs"][f"{fname}_a2"]["ms_median"] / a["ms_median"], 4),
            "control_b_in_a_median_vs_a_median": round(res["legs"][f"{fname}_b_in_a"]["ms_median"] / a["ms_median"], 4),
            "b_in_a_within_a_spread": res["legs"][f"{fname}_b_in_a"]["ms_median"] <= a["ms_max"]}
        for leg, _, roi in LEGS[1:]:
            r = res["legs"][f"{fname}_{leg}"]
            against = {"c": "g_c", "d": "g_c", "e": "g_e"}.get(leg)
            res["per_task"][f"{fname}_{leg}"] = {
                "tasks_vs_a": round(r["tasks"] / a["tasks"], 5), "ms_vs_a": round(r["ms_median"] / a["ms_median"], 5),
                "us_per_1000_tasks": round(1e6 * r["ms_median"] / r["tasks"], 3),
                "a_us_per_1000_tasks": round(1e6 * a["ms_median"] / a["tasks"], 3),
                "speedup_over_g": (round(res["legs"][f"{fname}_{against}"]["ms_median"] / r["ms_median"], 3)
                                   if against else None)}
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
        for name, roi, kernel in (("no_roi", None, "latency (AUTO)"),
                                  ("whole_frame_roi", (0, 0, w, h), "persistent (a ROI launch has no latency kernel)"),
                                  ("roi_224", ((w - 224) // 2, (h - 224) // 2, 224, 224), "persistent")):
            ow, oh = (w, h) if roi is None else roi[2:]
            out = torch.empty((1, 3, oh, ow), dtype=torch.uint8, device="cuda")
            t = []
            for i in range(iters + 5):
                t0 = time.perf_counter()
                gd.decode_rgb([data], out=out, rois=None if roi is None else [roi])
                gd.sync()
                if i >= 5:
                    t.append((time.perf_counter() - t0) * 1e3)
            res[name] = {"roi": list(roi) if roi else None, "ms_per_image_median": round(statistics.median(t), 4),
                         "ms_per_image_min": round(min(t), 4), "pixel_kernel": kernel,
                         "pixel_tasks": hjd.roi_geometry(w, h, info.sampling, 1, roi or (0, 0, w, h))[0]}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warm-rounds", type=int, default=3, help="untimed interleaved rounds before the timed ones")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "roi_decode_ab.json"))
    args = ap.parse_args()
    import torch
    import ocljpegdecoder_amd as hjd
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = hjd.Context(0)
    result = {"tool": "tools/roi_decode_ab.py", "utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
              "device": torch.cuda.get_device_name(0), "width": W, "height": H, "frames": args.frames,
              "rounds": args.rounds, "warm_rounds": args.warm_rounds, "input": "int16 zigzag",
              "kernel": "persistent, shape-default launch",
              "method": "untimed interleaved warm rounds of every leg, then interleaved rounds of one event-timed "
                        "launch per leg (the decode-then-slice routes in the same rounds); every ROI output checked "
                        "against the slice of the whole-frame output before and after timing",
              "d16_gather": list(ctx.d16_gather()), "samplings": {}}
    for sname, s in (("4:2:0", hjd.YUV420), ("4:4:4", hjd.YUV444)):
        r = run_sampling(torch, hjd, ctx, dev, s, args.frames, args.rounds, args.warm_rounds)
        result["samplings"][sname] = r
        for name, leg in r["legs"].items():
            print(f"{sname} {name:16s} {leg['ms_median']:8.3f} ms (median)  tasks {leg['tasks']:9d}  "
                  f"{leg['algorithmic_bytes'] / 1e6:10.1f} MB  spread {leg['spread']:.3f}", file=sys.stderr, flush=True)
        print(sname, "holds", json.dumps(r["holds"]), file=sys.stderr, flush=True)
    result["fhd_gpu_decoder"] = fhd_gpu_decoder(torch, hjd, ctx)
    print("fhd", json.dumps(result["fhd_gpu_decoder"]), file=sys.stderr, flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"roi_decode_ab": "ok", "file": os.path.relpath(args.out, REPO)}))


if __name__ == "__main__":
    main()

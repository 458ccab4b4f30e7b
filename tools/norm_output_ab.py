"""A/B of the normalised float outputs (OUT_RGB_PLANAR_F16 / _F32) against the
uint8 planar decode and against the two-pass route they replace, one device,
same run.

    python tools/norm_output_ab.py [--frames 256] [--rounds 12] [--out profiles/norm_output_ab.json]

Persistent kernel, 3840x2160 frames, 4:2:0 and 4:4:4, int16 zigzag input,
ImageNet mean / std.  All legs of a sampling decode the same coefficient
buffer; after untimed interleaved warm rounds of every leg they are timed with
device events in interleaved rounds (one run of each leg per round), so drift
hits all alike.

Legs (per sampling):
  a          OUT_RGB_PLANAR, uint8 (N, 3, H, W)
  b          OUT_RGB_PLANAR_F16, one launch
  c          OUT_RGB_PLANAR_F32, one launch
  d16_*, d32_*  the route b / c replace: leg a, then torch's conversion of its
             output into a preallocated tensor of the dtype, every way listed
             in CONVERTERS that this torch accepts; the fastest (lowest
             median) is the route a fused leg is compared with, and its name
             is recorded
  a_s2       leg a at scale 2 (the whole 1920x1080 grid), for the e legs
  e16, e32   b and c with a centred 224x224 ROI at scale 2
  f16_*, f32_*  the route e replaces: a_s2, slice, convert into a preallocated
             (N, 3, 224, 224) tensor

Per leg: ms (minimum, median, maximum over the rounds), the algorithmic bytes
(coefficient bytes read plus bytes written; a two-pass leg adds the bytes its
second pass reads and writes), bytes per source pixel and the fraction of
8 TB/s they amount to.  `holds`: each fused leg's median against the median of
the fastest two-pass route of the same run (the condition: fused < two-pass);
`f16_vs_u8` is recorded, not a condition.  Before timing, b must equal c
rounded to half bit for bit, and c must agree with the two-pass float32 result
to 1e-6 relative (torch's route rounds twice).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from out_format_ab import H, W, POOL, qtables, synth_frame   # noqa: E402  (the same synthetic frames)

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
ROI_E = ((W // 2 - 224) // 2, (H // 2 - 224) // 2, 224, 224)   # on the scale-2 grid; x % 4 == 0
HBM_BYTES_PER_MS = 8e9                                          # 8 TB/s


def converters(torch):
    """Ways to write a * x + b of a uint8 tensor x into a preallocated float
    tensor `out` (a, b: float32, broadcast over (1, 3, 1, 1))."""
    return [
        ("addcmul", lambda x, a, b, out: torch.addcmul(b, x, a, out=out)),
        ("mul_out_add_", lambda x, a, b, out: torch.mul(x, a, out=out).add_(b)),
        ("copy_mul_add_", lambda x, a, b, out: out.copy_(x).mul_(a).add_(b)),
    ]


def run_sampling(torch, hjd, ctx, dev, sampling, nf, rounds, warm_rounds):
    qt = qtables()
    mw, mh, bpm, _ = hjd.mcu_geometry(W, H, sampling)
    nblk = mw * mh * bpm
    coefs = torch.empty((nf, nblk, 64), dtype=torch.int16, device=dev)
    for i in range(min(POOL, nf)):
        coefs[i] = synth_frame(torch, hjd, nblk, sampling, qt, seed=7000 + i, dev=dev)
    for i in range(POOL, nf):
        coefs[i].copy_(coefs[i % POOL])
    a_np, b_np = hjd.norm_constants(MEAN, STD)
    a_t = torch.tensor(a_np, device=dev).view(1, 3, 1, 1)
    b_t = torch.tensor(b_np, device=dev).view(1, 3, 1, 1)
    tdt = {"u8": torch.uint8, "f16": torch.float16, "f32": torch.float32}
    fmt = {"u8": hjd.OUT_RGB_PLANAR, "f16": hjd.OUT_RGB_PLANAR_F16, "f32": hjd.OUT_RGB_PLANAR_F32}
    # (leg, element, scale, roi)
    fused = [("a", "u8", 1, None), ("b", "f16", 1, None), ("c", "f32", 1, None),
             ("a_s2", "u8", 2, None), ("e16", "f16", 2, ROI_E), ("e32", "f32", 2, ROI_E)]
    plans, outs = {}, {}
    for leg, el, scale, roi in fused:
        ow, oh = hjd.FrameSpec(W, H, sampling, out_format=fmt[el], roi=roi).out_size(scale)
        outs[leg] = torch.zeros((nf, 3, oh, ow), dtype=tdt[el], device=dev)
        fb = 3 * oh * ow * outs[leg].element_size()
        specs = [hjd.FrameSpec(W, H, sampling, coef_offset=i * nblk, out_offset=i * fb, qt_index=(0, 1, 2),
                               out_format=fmt[el], roi=roi) for i in range(nf)]
        plans[leg] = hjd.Plan(ctx, specs, hjd.IN_Q16_ZIGZAG, qtables=qt, scale=scale,
                              normalize=(a_np, b_np) if el != "u8" else None)
        plans[leg].set_kernel(hjd.KERNEL_PERSISTENT)
    stream = torch.cuda.current_stream()
    x, y, rw, rh = ROI_E
    conv_out = {"d16": torch.zeros((nf, 3, H, W), dtype=torch.float16, device=dev),
                "d32": torch.zeros((nf, 3, H, W), dtype=torch.float32, device=dev),
                "f16": torch.zeros((nf, 3, rh, rw), dtype=torch.float16, device=dev),
                "f32": torch.zeros((nf, 3, rh, rw), dtype=torch.float32, device=dev)}

    def launch(leg):
        plans[leg].launch(coefs, outs[leg], stream)

    def two_pass(route, fn):
        if route[0] == "d":
            launch("a")
            fn(outs["a"], a_t, b_t, conv_out[route])
        else:
            launch("a_s2")
            fn(outs["a_s2"][:, :, y:y + rh, x:x + rw], a_t, b_t, conv_out[route])

    # which converters this torch accepts (tried on a small tensor, checked against float64)
    small = torch.arange(256, dtype=torch.uint8, device=dev).repeat(3).view(1, 3, 16, 16)
    want = small.double() * a_t.double() + b_t.double()
    usable = []
    for name, fn in converters(torch):
        try:
            for dt, tol in ((torch.float32, 1e-6), (torch.float16, 2e-3)):
                o = torch.zeros((1, 3, 16, 16), dtype=dt, device=dev)
                fn(small, a_t, b_t, o)
                if not torch.allclose(o.double(), want, rtol=tol, atol=tol):
                    raise RuntimeError("wrong result")
            usable.append((name, fn))
        except Exception as e:   # noqa: BLE001  (a converter this torch refuses is left out, and named)
            print(f"converter {name}: not usable ({type(e).__name__}: {str(e)[:80]})", file=sys.stderr, flush=True)
    if not usable:
        raise SystemExit("no two-pass converter works")
    jobs = [(leg, (lambda leg=leg: launch(leg))) for leg, *_ in fused]
    for route in ("d16", "d32", "f16", "f32"):
        for name, fn in usable:
            jobs.append((f"{route}_{name}", (lambda route=route, fn=fn: two_pass(route, fn))))

    for _ in range(max(1, warm_rounds)):
        for _, job in jobs:
            job()
    torch.cuda.synchronize()
    # consistency: F16 is F32 rounded to half; F32 agrees with torch's route; the ROI is the slice
    for k in range(0, nf, max(1, nf // 8)):
        if not torch.equal(outs["b"][k].view(torch.int16), outs["c"][k].to(torch.float16).view(torch.int16)):
            raise SystemExit("F16 output is not the F32 output rounded to half")
        ref = conv_out["d32"][k]
        if not torch.allclose(outs["c"][k], ref, rtol=1e-6, atol=1e-6):
            raise SystemExit("F32 output disagrees with the two-pass result")
        if not torch.allclose(outs["e32"][k], conv_out["f32"][k], rtol=1e-6, atol=1e-6):
            raise SystemExit("the ROI F32 output disagrees with slice + convert")
        if not torch.equal(outs["e16"][k].view(torch.int16), outs["e32"][k].to(torch.float16).view(torch.int16)):
            raise SystemExit("the ROI F16 output is not the F32 one rounded to half")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    ms = {name: [] for name, _ in jobs}
    for _ in range(rounds):
        for name, job in jobs:
            ms[name].append(timed(job))

    src_px = nf * W * H
    res = {"legs": {}, "holds": {}, "converters_usable": [n for n, _ in usable]}

    def put(name, v, alg_bytes, extra):
        med = statistics.median(v)
        d = {"ms_min": round(min(v), 4), "ms_median": round(med, 4), "ms_max": round(max(v), 4),
             "ms_rounds": [round(t, 4) for t in v], "algorithmic_bytes": alg_bytes,
             "bytes_per_source_px": round(alg_bytes / src_px, 4),
             "fraction_of_8TBps": round(alg_bytes / med / HBM_BYTES_PER_MS, 4)}
        d.update(extra)
        res["legs"][name] = d

    written = {leg: outs[leg].numel() * outs[leg].element_size() for leg, *_ in fused}
    for leg, el, scale, roi in fused:
        put(leg, ms[leg], plans[leg].coef_bytes + written[leg],
            {"element": el, "scale": scale, "roi": list(roi) if roi else None, "tasks": plans[leg].tasks,
             "out_shape": list(outs[leg].shape), "launch_shape": plans[leg].launch_shape()})
    for route in ("d16", "d32", "f16", "f32"):
        first = "a" if route[0] == "d" else "a_s2"
        o = conv_out[route]
        second = o.numel() * (1 + o.element_size())      # the second pass reads the bytes and writes the floats
        for name, _ in usable:
            put(f"{route}_{name}", ms[f"{route}_{name}"], plans[first].coef_bytes + written[first] + second,
                {"route": f"leg {first}" + (", slice" if route[0] == "f" else "") + f", {name} into a preallocated tensor",
                 "second_pass_bytes": second})
    for fused_leg, route in (("b", "d16"), ("c", "d32"), ("e16", "f16"), ("e32", "f32")):
        best = min((res["legs"][f"{route}_{n}"]["ms_median"], n) for n, _ in usable)
        f = res["legs"][fused_leg]
        res["holds"][fused_leg] = {"fused_ms_median": f["ms_median"], "fused_ms_max": f["ms_max"],
                                   "two_pass": f"{route}_{best[1]}", "two_pass_ms_median": best[0],
                                   "fused_vs_two_pass": round(f["ms_median"] / best[0], 4),
                                   "fused_below_two_pass": f["ms_median"] < best[0]}
    a = res["legs"]["a"]
    res["f16_vs_u8"] = round(res["legs"]["b"]["ms_median"] / a["ms_median"], 4)
    res["f32_vs_u8"] = round(res["legs"]["c"]["ms_median"] / a["ms_median"], 4)
    for p in plans.values():
        p.close()
    del coefs, outs, conv_out
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warm-rounds", type=int, default=3, help="untimed interleaved rounds before the timed ones")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "norm_output_ab.json"))
    args = ap.parse_args()
    import torch
    import ocljpegdecoder_amd as hjd
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = hjd.Context(0)
    result = {"tool": "tools/norm_output_ab.py", "utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
              "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "width": W, "height": H,
              "frames": args.frames, "rounds": args.rounds, "warm_rounds": args.warm_rounds, "input": "int16 zigzag",
              "mean": list(MEAN), "std": list(STD), "roi_e_on_scale_2_grid": list(ROI_E),
              "kernel": "persistent, shape-default launch",
              "method": "untimed interleaved warm rounds of every leg, then interleaved rounds of one event-timed run "
                        "per leg; the two-pass routes (decode to uint8, then torch's conversion into a preallocated "
                        "tensor) in the same rounds, every converter this torch accepts",
              "d16_gather": list(ctx.d16_gather()), "samplings": {}}
    for sname, s in (("4:2:0", hjd.YUV420), ("4:4:4", hjd.YUV444)):
        r = run_sampling(torch, hjd, ctx, dev, s, args.frames, args.rounds, args.warm_rounds)
        result["samplings"][sname] = r
        for name, leg in r["legs"].items():
            print(f"{sname} {name:22s} {leg['ms_median']:9.3f} ms (median)  {leg['bytes_per_source_px']:7.3f} B/px  "
                  f"{leg['fraction_of_8TBps']:.3f} of 8 TB/s", file=sys.stderr, flush=True)
        print(sname, "holds", json.dumps(r["holds"]), "f16_vs_u8", r["f16_vs_u8"], file=sys.stderr, flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"norm_output_ab": "ok", "file": os.path.relpath(args.out, REPO)}))


if __name__ == "__main__":
    main()

"""A/B of the fused kernel's four output formats on one device, same run.

    python tools/out_format_ab.py [--frames 256] [--rounds 30] [--out profiles/out_formats_ab.json]

Persistent kernel, 3840x2160, 4:2:0 and 4:4:4, int16 zigzag input.  The four
formats (BGRX, BGR24, RGB24, planar RGB) decode the same coefficient buffer;
after warm launches of each (untimed interleaved rounds, until the clocks have
settled) they are timed with device events in interleaved rounds (one launch
of each format per round), so drift hits all four alike.
Before any number is reported every format's output is checked against the
BGRX output of the same run, permuted.

Per format: ms per launch (minimum and median over the rounds), Mpx/s, the
algorithmic bytes (coefficient bytes + 4 or 3 B/px) and their fraction of
8 TB/s.  The three 3-byte formats move the same bytes, and the BGR24 kernel is
the yardstick for the two RGB ones; `spread` is each format's (max - min) / min
over the rounds, the noise a difference has to exceed.
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

W, H = 3840, 2160
PEAK = 8e12   # B/s, MI355X HBM3E
POOL = 8      # distinct synthetic frames, repeated over the batch

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
          7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
          39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def qtables():
    """Annex K tables in file (zigzag) order."""
    lum = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55,
                    14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
    chr_ = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
                     24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)
    return np.stack([lum, chr_, chr_])[:, ZIGZAG].astype(np.int32)


def synth_frame(torch, hjd, nblk, sampling, qt, seed, dev):
    """Quantised zigzag coefficients of one synthetic frame (bounded samples ->
    FDCT -> quantise: inside the decoder's legal domain), made on the device."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    k = torch.arange(8, device=dev, dtype=torch.float32)
    cc = torch.where(k == 0, 1 / np.sqrt(2), 1.0)
    m = torch.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * cc[:, None] / 2
    yy, xx = torch.meshgrid(torch.arange(8, device=dev), torch.arange(8, device=dev), indexing="ij")
    base = torch.randint(-100, 100, (nblk, 1, 1), generator=g, device=dev).float()
    grad = torch.randn((nblk, 2, 1, 1), generator=g, device=dev) * 6
    pix = (base + grad[:, 0] * yy + grad[:, 1] * xx + torch.randn((nblk, 8, 8), generator=g, device=dev) * 20)
    F = torch.einsum("ux,nxy,vy->nuv", m, pix.clamp(-128, 127), m).reshape(nblk, 64)
    zz = torch.tensor(ZIGZAG, device=dev)
    qnat = torch.zeros((3, 64), device=dev)
    qnat[:, zz] = torch.from_numpy(qt).float().to(dev)
    comp = torch.from_numpy(hjd.block_components(sampling, nblk)).to(dev)
    return torch.round(F / qnat[comp])[:, zz].to(torch.int16).contiguous()


def check_against_bgrx(torch, hjd, name, out, bgrx, nf, chunk=16):
    """out == bgrx (nf, H, W, 4 bytes) permuted to the format's layout."""
    for a in range(0, nf, chunk):
        b = min(nf, a + chunk)
        ref = bgrx[a:b]
        if name == "bgr24":
            ok = torch.equal(out[a:b].view(b - a, H, W, 3), ref[..., :3])
        elif name == "rgb24":
            ok = torch.equal(out[a:b].view(b - a, H, W, 3), ref[..., [2, 1, 0]])
        else:
            ok = torch.equal(out[a:b].view(b - a, 3, H, W), ref[..., [2, 1, 0]].permute(0, 3, 1, 2))
        if not ok:
            raise SystemExit(f"{name}: frames {a}..{b - 1} differ from the BGRX output of this run")


def run_sampling(torch, hjd, ctx, dev, sampling, nf, rounds, warm_rounds):
    qt = qtables()
    mw, mh, bpm, _ = hjd.mcu_geometry(W, H, sampling)
    nblk = mw * mh * bpm
    coefs = torch.empty((nf, nblk, 64), dtype=torch.int16, device=dev)
    for i in range(min(POOL, nf)):
        coefs[i] = synth_frame(torch, hjd, nblk, sampling, qt, seed=7000 + i, dev=dev)
    for i in range(POOL, nf):
        coefs[i].copy_(coefs[i % POOL])
    formats = [("bgrx", hjd.OUT_BGRX), ("bgr24", hjd.OUT_BGR24), ("rgb24", hjd.OUT_RGB24),
               ("rgb_planar", hjd.OUT_RGB_PLANAR)]
    plans, outs = {}, {}
    for name, fmt in formats:
        pitch = hjd.default_pitch(W, fmt)
        frame_bytes = pitch * hjd.backend.out_rows(H, fmt)
        outs[name] = torch.zeros((nf, frame_bytes), dtype=torch.uint8, device=dev)
        specs = [hjd.FrameSpec(W, H, sampling, coef_offset=i * nblk, out_offset=i * frame_bytes, out_pitch=pitch,
                               qt_index=(0, 1, 2), out_format=fmt) for i in range(nf)]
        plans[name] = hjd.Plan(ctx, specs, hjd.IN_Q16_ZIGZAG, qtables=qt)
        plans[name].set_kernel(hjd.KERNEL_PERSISTENT)
    stream = torch.cuda.current_stream()
    for _ in range(max(1, warm_rounds)):   # warm launches of each, interleaved like the timed ones
        for name, _ in formats:
            plans[name].launch(coefs, outs[name], stream)
    torch.cuda.synchronize()
    bgrx = outs["bgrx"].view(nf, H, W, 4)
    for name, _ in formats[1:]:
        check_against_bgrx(torch, hjd, name, outs[name], bgrx, nf)
    ms = {name: [] for name, _ in formats}
    for _ in range(rounds):
        for name, _fmt in formats:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            plans[name].launch(coefs, outs[name], stream)
            e1.record(stream)
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    for name, _ in formats[1:]:   # the timed launches wrote the same pixels
        check_against_bgrx(torch, hjd, name, outs[name], bgrx, nf)
    px = nf * W * H
    res = {}
    for name, fmt in formats:
        best, med = min(ms[name]), statistics.median(ms[name])
        nbytes = plans[name].coef_bytes + px * hjd.OUT_BYTES[fmt]
        res[name] = {"ms_min": round(best, 4), "ms_median": round(med, 4), "ms_rounds": [round(v, 4) for v in ms[name]],
                     "spread": round((max(ms[name]) - best) / best, 4),
                     "mpx_per_s": round(px / best / 1e3, 1), "mpx_per_s_median": round(px / med / 1e3, 1),
                     "algorithmic_bytes": int(nbytes), "bytes_per_px": round(nbytes / px, 3),
                     "frac_of_8TBps": round(nbytes / (best * 1e-3) / PEAK, 4),
                     "launch_shape": plans[name].launch_shape()}
    for name in ("rgb24", "rgb_planar"):
        res[name]["vs_bgr24"] = round(res["bgr24"]["ms_min"] / res[name]["ms_min"], 4)
        res[name]["vs_bgr24_median"] = round(res["bgr24"]["ms_median"] / res[name]["ms_median"], 4)
    for p in plans.values():
        p.close()
    del coefs, outs, bgrx
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warm-rounds", type=int, default=5, help="untimed interleaved rounds before the timed ones")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "out_formats_ab.json"))
    args = ap.parse_args()
    import torch
    import ocljpegdecoder_amd as hjd
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = hjd.Context(0)
    result = {"tool": "tools/out_format_ab.py", "utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
              "device": torch.cuda.get_device_name(0), "width": W, "height": H, "frames": args.frames,
              "rounds": args.rounds, "warm_rounds": args.warm_rounds, "input": "int16 zigzag", "kernel": "persistent, shape-default launch",
              "method": "warm launches of every format (untimed interleaved rounds), then interleaved rounds of one event-timed launch per format; "
                        "every format checked against this run's BGRX output (permuted) before and after timing",
              "d16_gather": list(ctx.d16_gather()), "samplings": {}}
    for sname, s in (("4:2:0", hjd.YUV420), ("4:4:4", hjd.YUV444)):
        result["samplings"][sname] = run_sampling(torch, hjd, ctx, dev, s, args.frames, args.rounds,
                                                      args.warm_rounds)
        for name, r in result["samplings"][sname].items():
            print(f"{sname} {name:10s} {r['ms_min']:8.3f} ms  {r['mpx_per_s']:10.1f} Mpx/s  "
                  f"{r['frac_of_8TBps']:.3f} of 8 TB/s  spread {r['spread']:.3f}", file=sys.stderr, flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out_format_ab": "ok", "file": os.path.relpath(args.out, REPO)}))


if __name__ == "__main__":
    main()

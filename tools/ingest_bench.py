"""What the input format costs: the four IQ formats of the C ABI (FMD_IQ_F32 / U8 / S8 / S16, include/fmd.h) through
the same batch geometry on one box, overlapped calls (concurrency 2) consumed two calls late as bench.py runs them.

  channels: 8192 channels x 65 536 samples, 2.4 MS/s, D = 11 (the headline), one input row per channel
  captures: 32 captures x 256 stations = 8192 channels, table_size 256 (config 3 scaled out)
  config5:  4096 channels, 10 MS/s, D = 46, 4096-tap IF filter (BASELINE configs[4])

Per geometry the formats are visited twice in alternation (f32, u8, s8, s16, f32, u8, s8, s16); per format: ms per
step of each visit, MS/s of the best, the IF stage's own ms (a short run at profiling level 1: the FIR kernel's own
start and stop events inside the overlapped pipeline) and the fraction of the HBM peak that is on the bytes of that
format.  The input is generated on the device by the signal
generator (float) and quantised with torch: round(x * 32767), round(x * 127), clipped; bytes: round((x + 1) * 127.5).
One JSON line, also written to profiles/ingest_formats.json.

    python tools/ingest_bench.py --steps 240 --warmup 8 [--geometries channels,captures,config5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402
from tools import fmsig_py  # noqa: E402

N, LAG, RING = 65536, 2, 3
HBM_PEAK_GBS = 8000.0  # HBM3E 8.0 TB/s spec, as bench.py
FORMATS = ["f32", "u8", "s8", "s16"]
GEOMETRIES = {
    "channels": dict(fs=2.4e6, D=11, order=0, table=0, C=8192, G=0),
    "captures": dict(fs=2.4e6, D=11, order=0, table=256, C=8192, G=32),
    "config5": dict(fs=10e6, D=46, order=4096, table=0, C=4096, G=0),
}


def float_ring(g):
    """[RING][rows][N][2] float32 on the device: a station per channel, or six stations per capture"""
    if not g["G"]:
        gen = fmsig_py.DeviceGenerator([fmsig_py.channel_params(g["fs"], c) for c in range(g["C"])], "cuda")
        iq = torch.empty((RING, g["C"], N, 2), dtype=torch.float32, device="cuda")
        for r in range(RING):
            gen.generate(iq[r], r * N, N)
        return iq
    offs = (-600e3, -360e3, -150e3, 75e3, 300e3, 600e3)
    iq = torch.empty((RING, g["G"], N, 2), dtype=torch.float32, device="cuda")
    tmp = torch.empty((len(offs), N, 2), dtype=torch.float32, device="cuda")
    for cap in range(g["G"]):
        st = [fmsig_py.default_params(g["fs"], f_offset=f0, amp=0.12, noise_sigma=0.004, seed=50 + i + 16 * cap,
                                      pi=0x5000 + i + 16 * cap, ps="CAP%05d" % (i + 16 * cap),
                                      f_left=500.0 + 300 * i + 7 * cap) for i, f0 in enumerate(offs)]
        gen = fmsig_py.DeviceGenerator(st, "cuda")
        for r in range(RING):
            gen.generate(tmp, r * N, N)
            iq[r, cap] = tmp.sum(dim=0)
    return iq


def quantise(x, fmt):
    if fmt == "f32":
        return x
    if fmt == "s16":
        return torch.clamp(torch.round(x * 32767.0), -32768, 32767).to(torch.int16)
    if fmt == "s8":
        return torch.clamp(torch.round(x * 127.0), -128, 127).to(torch.int8)
    return torch.clamp(torch.round((x + 1.0) * 127.5), 0, 255).to(torch.uint8)


def make_batch(pkg, g):
    C, table = g["C"], g["table"]
    shifts = (np.arange(C, dtype=np.int32) % table) - table // 2 if g["G"] else None
    b = pkg.Batch(pkg.make_params(g["fs"], 0.0 if g["G"] else -0.15 * g["fs"], 48000.0, 15000.0, g["D"],
                                  table_size=table, if_filter_order=g["order"]),
                  C, tuning_shifts=shifts, record_callbacks=False)
    if g["G"]:
        b.set_channels_per_capture(C // g["G"])
    b.set_concurrency(2)
    return b


def run(pkg, g, iq, fmt_code, steps, warmup, profile=False):
    b = make_batch(pkg, g)
    if profile:
        b.set_profiling(1)
    a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
    audio = [torch.empty((g["C"], a_stride), dtype=torch.float32, device="cuda") for _ in range(LAG + 3)]
    s = torch.cuda.current_stream().cuda_stream
    t0 = None
    for j in range(warmup + steps):
        if j == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        b.process_device(iq[j % RING].data_ptr(), N, N, audio[j % len(audio)].data_ptr(), a_stride, s, fmt=fmt_code)
        if j >= LAG:
            b.wait(stream=s, lag=LAG)
            b.collect_rds_array(cap=4 * g["C"], stream=s, lag=LAG)
    b.wait(stream=s)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    fir = b.stage_ms()[0]["if_fir"] if profile else None
    b.close()
    return ms, fir


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--profile-steps", type=int, default=32)
    ap.add_argument("--geometries", default="channels,captures,config5")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_formats.json"))
    args = ap.parse_args()
    pkg = load_package()
    codes = {"f32": pkg.FMD_IQ_F32, "u8": pkg.FMD_IQ_U8, "s8": pkg.FMD_IQ_S8, "s16": pkg.FMD_IQ_S16}
    res = {"tool": "ingest_bench", "samples": N, "lag": LAG, "steps": args.steps, "warmup": args.warmup,
           "order_of_visits": FORMATS * 2, "hbm_peak_gbs": HBM_PEAK_GBS, "geometries": {}}
    for name in [x for x in args.geometries.split(",") if x]:
        g = GEOMETRIES[name]
        base = float_ring(g)
        rings = {f: quantise(base, f).contiguous() for f in FORMATS}
        torch.cuda.synchronize()
        rows = base.shape[1]
        out = {"channels": g["C"], "input_rows": rows, "sample_rate_if": g["fs"], "downsample": g["D"],
               "if_filter_order": g["order"] or 8 * g["D"], "formats": {}}
        visits = {f: [] for f in FORMATS}
        for _ in range(2):  # alternated: every format once per round
            for f in FORMATS:
                ms, _ = run(pkg, g, rings[f], codes[f], args.steps, args.warmup)
                visits[f].append(round(ms, 4))
        for f in FORMATS:
            _, fir = run(pkg, g, rings[f], codes[f], args.profile_steps, args.warmup, profile=True)
            in_bytes = rows * N * pkg.IQ_BYTES[codes[f]]
            best = min(visits[f])
            gbs = in_bytes / (fir * 1e-3) / 1e9
            out["formats"][f] = {"ms_per_step": visits[f], "ms_samples_per_s": round(g["C"] * N / (best * 1e-3) / 1e6, 1),
                                 "if_fir_ms": round(fir, 4), "input_bytes_per_call": in_bytes,
                                 "if_input_gb_per_s": round(gbs, 1), "if_hbm_frac": round(gbs / HBM_PEAK_GBS, 4)}
        f32 = min(visits["f32"])
        for f in FORMATS[1:]:
            out["formats"][f]["vs_f32"] = round(f32 / min(visits[f]) - 1.0, 4)
        res["geometries"][name] = out
        del base, rings
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

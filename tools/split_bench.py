"""What the band splitter costs and what it buys (fmd_split_*, include/fmd.h).

(a) The splitter alone: ms per call and GB/s against the byte floor -- input once plus output once, (bytes per input
    sample + 8 B / R) bytes per input sample -- at 32 captures x 262 144 samples, R = 4, 5 bands, and 16 x 524 288,
    R = 8, 10 bands; float, s16 and s8 input.
(b) What it is for, two ways on the same wideband captures and the same stations (8 per band): decoded DIRECTLY, a
    batch at the wideband rate with the reference's IF order 8 D (D = 11 R, so its baseband rate is the split path's),
    channels_per_capture stations on every capture, in calls of FMD_MAX_BLOCK samples; and SPLIT, the splitter plus
    a batch at fs / R with a capture map, both on one stream.  Reported: ms per call and the stations decoded in real time per GPU, stations x (signal
    time of a call / time of a call).  The input is noise: no time of either path depends on what the samples hold.

Device events around `--steps` (the splitter alone: `--alone-steps`) back-to-back calls after `--warmup` untimed
ones; the formats of (a) and the two ways of (b) alternate `--visits` times and every visit is reported; rates are of
the better visit.  Prints one JSON line and writes it to --out.

    python tools/split_bench.py --steps 20 --warmup 3 --out profiles/split.json

--real: a real-sampled capture two ways at the same two geometries -- the real splitter on
FMD_REAL_S16 / _F32 input, and what a host had to do without it, the complex splitter on the same samples with a zero Q
interleaved (FMD_IQ_S16 / _F32, twice the bytes), same G, samples, R, B and shifts; the four alternate `--visits`
times, every visit is reported.  Plus one direct-sampling geometry, reported and compared with nothing: 4 captures x
4 194 304 samples at 122.88 MS/s, R 48, K 384, T 1024, 12 bands.

    python tools/split_bench.py --real --out profiles/split_real.json
"""
import argparse
import json
import os
import sys
from importlib import import_module

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

FS_BAND, D_BAND, T_BAND = 2.4e6, 11, 24     # the batch behind the splitter: the headline geometry
GEOMETRIES = [(4, 32, 262144, 5), (8, 16, 524288, 10)]  # (R, captures, samples, bands)
STATIONS_PER_BAND = 8


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def band_shifts(R, B):
    """B band centres spread over the capture, on the raster of 100 kHz"""
    T = int(round(FS_BAND * R / 100e3))
    span = T // 2 - 10
    return T, [int(round(-span + 2 * span * b / (B - 1))) for b in range(B)]


def inputs(G, n):
    torch.manual_seed(1)
    f32 = (0.1 * torch.randn((G, 2 * n), dtype=torch.float32, device="cuda")).contiguous()
    s16 = torch.clamp(f32 * 32767.0, -32768, 32767).to(torch.int16).contiguous()
    s8 = torch.clamp(f32 * 127.0, -128, 127).to(torch.int8).contiguous()
    return {"f32": (f32, 8), "s16": (s16, 4), "s8": (s8, 2)}


DIRECT_SAMPLING = {"fs": 122.88e6, "R": 48, "K": 384, "T": 1024, "captures": 4, "samples": 4194304, "bands": 12}


def real_inputs(G, n):
    """noise as real samples, and the same samples with a zero Q interleaved"""
    torch.manual_seed(1)
    f32 = (0.1 * torch.randn((G, n), dtype=torch.float32, device="cuda")).contiguous()
    s16 = torch.clamp(f32 * 32767.0, -32768, 32767).to(torch.int16).contiguous()
    zq = lambda t: torch.stack([t, torch.zeros_like(t)], dim=2).reshape(G, 2 * n).contiguous()
    return {"real_s16": (s16, 2), "zero_q_s16": (zq(s16), 4), "real_f32": (f32, 4), "zero_q_f32": (zq(f32), 8)}


def main_real(args, split):
    stream = torch.cuda.current_stream().cuda_stream
    res = {"alone_steps": args.alone_steps, "warmup": args.warmup, "visits": args.visits,
           "device": torch.cuda.get_device_name(0), "compare": [], "direct_sampling": []}
    for R, G, n, B in GEOMETRIES:
        G = max(1, G // args.scale)
        fs = FS_BAND * R
        T, shifts = band_shifts(R, B)
        x = real_inputs(G, n)
        sp = {True: split.Splitter(fs, R, G, [shifts] * G, table_size=T, real=True),
              False: split.Splitter(fs, R, G, [shifts] * G, table_size=T)}
        out = torch.empty((G * B, sp[True].out_stride(n)), dtype=torch.complex64, device="cuda")
        ms = {name: [] for name in x}
        for _ in range(args.visits):
            for name, (t, esz) in x.items():
                s_ = sp[name.startswith("real")]
                ms[name].append(timed(lambda: s_.process(t, n, out=out, stream=stream), args.alone_steps, args.warmup))
        entry = {"R": R, "captures": G, "samples": n, "bands": B, "table_size": T,
                 "ms_per_call": {k: [round(v, 4) for v in vs] for k, vs in ms.items()}}
        for fmt in ("s16", "f32"):
            r, z = ms["real_" + fmt], ms["zero_q_" + fmt]
            entry["real_over_zero_q_" + fmt] = round(min(r) / min(z), 4)
            entry["zero_q_spread_" + fmt] = round((max(z) - min(z)) / min(z), 4)
            entry["real_slower_than_every_zero_q_visit_" + fmt] = bool(min(r) > max(z))
        res["compare"].append(entry)
        for s_ in sp.values():
            s_.close()
    d = DIRECT_SAMPLING
    G, n, B = max(1, d["captures"] // args.scale), d["samples"], d["bands"]
    span = d["T"] // 2 - 40
    shifts = [int(round(-span + 2 * span * b / (B - 1))) for b in range(B)]
    sp = split.Splitter(d["fs"], d["R"], G, [shifts] * G, filter_order=d["K"], table_size=d["T"], real=True)
    out = torch.empty((G * B, sp.out_stride(n)), dtype=torch.complex64, device="cuda")
    x = real_inputs(G, n)
    for name in ("real_s16", "real_f32"):
        t, esz = x[name]
        v = [timed(lambda: sp.process(t, n, out=out, stream=stream), max(1, args.alone_steps // 20), args.warmup)
             for _ in range(args.visits)]
        floor = G * n * (esz + 8.0 * B / d["R"])
        res["direct_sampling"].append(dict(d, captures=G, input=name, tile_samples=sp.tile_samples,
                                           ms_per_call=[round(a, 4) for a in v], floor_bytes=int(floor),
                                           GBps_of_floor_bytes=round(floor / min(v) / 1e6, 1),
                                           signal_ms_per_call=round(n / d["fs"] * 1e3, 3)))
    sp.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--alone-steps", type=int, default=1000, help="calls of the splitter alone per timed window")
    ap.add_argument("--visits", type=int, default=2)
    ap.add_argument("--scale", type=int, default=1, help="divide captures by this (a rehearsal at a small size)")
    ap.add_argument("--real", action="store_true", help="real-sampled input against zero-Q complex input")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("split_bench: no GPU (nothing here is measured on a CPU)")
    pkg = load_package()
    split = import_module(pkg.__name__ + ".split")
    if args.real:
        line = json.dumps(main_real(args, split))
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
    stream = torch.cuda.current_stream().cuda_stream
    res = {"steps": args.steps, "alone_steps": args.alone_steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "alone": [],
           "decode": []}
    for R, G, n, B in GEOMETRIES:
        G = max(1, G // args.scale)
        fs = FS_BAND * R
        T, shifts = band_shifts(R, B)
        x = inputs(G, n)
        sp = split.Splitter(fs, R, G, [shifts] * G, table_size=T)
        out = torch.empty((G * B, sp.out_stride(n)), dtype=torch.complex64, device="cuda")
        # (a) alone
        alone = {name: [] for name in x}
        for _ in range(args.visits):  # the formats alternate; every visit is reported
            for name, (t, esz) in x.items():
                alone[name].append(timed(lambda: sp.process(t, n, out=out, stream=stream), args.alone_steps,
                                         args.warmup))
        for name, (t, esz) in x.items():
            ms = min(alone[name])
            floor = G * n * (esz + 8.0 * B / R)
            res["alone"].append({"R": R, "captures": G, "samples": n, "bands": B, "input": name,
                                 "ms_per_call": [round(v, 4) for v in alone[name]], "floor_bytes": int(floor),
                                 "GBps_of_floor_bytes": round(floor / ms / 1e6, 1),
                                 "input_MSps": round(G * n / ms / 1e3, 1)})
        # (b) the same stations, directly and split
        per_cap = B * STATIONS_PER_BAND
        C = G * per_cap
        # station s of band b sits (s - 3.5) * 200 kHz from the band's centre: shift in the band's raster of 100 kHz
        in_band = [int(2 * s - STATIONS_PER_BAND + 1) for s in range(STATIONS_PER_BAND)]
        direct_shifts = np.array([[bs + k for k in in_band] for bs in shifts] * G, np.int32).reshape(-1)
        split_shifts = np.array([in_band] * (G * B), np.int32).reshape(-1)
        f32 = x["f32"][0]
        blk = 65536  # FMD_MAX_BLOCK: a batch call takes no more; a band's share of a splitter call is one block
        entry = {"R": R, "fs": fs, "captures": G, "samples": n, "bands": B, "stations": C,
                 "direct_downsample": D_BAND * R, "direct_if_order": 8 * D_BAND * R,
                 "signal_ms_per_call": round(n / fs * 1e3, 3)}
        bd = None
        try:
            bd = pkg.Batch(pkg.make_params(fs, 0.0, 48000.0, 15000.0, D_BAND * R, table_size=T), C,
                           tuning_shifts=direct_shifts, record_callbacks=False)
            bd.set_channels_per_capture(per_cap)
        except pkg.FmdError as e:  # reported, not hidden: this geometry cannot be decoded directly at all
            entry["direct_error"] = str(e)
            bd = None
        bs_ = pkg.Batch(pkg.make_params(FS_BAND, 0.0, 48000.0, 15000.0, D_BAND, table_size=T_BAND), C,
                        tuning_shifts=split_shifts, record_callbacks=False)
        bs_.set_capture_map(np.arange(C, dtype=np.uint32) // STATIONS_PER_BAND, G * B)
        a_stride = (max(bs_.max_audio_floats(blk), bs_.max_audio_floats(n // R)) + 63) // 64 * 64
        audio = torch.empty((C, a_stride), dtype=torch.float32, device="cuda")

        def direct():
            for k in range(n // blk):
                bd.process_device(f32.data_ptr() + 8 * k * blk, n, blk, audio.data_ptr(), a_stride, stream)
            bd.collect_rds(stream=stream)

        def behind_split():
            _, m = sp.process(f32, n, out=out, stream=stream)
            bs_.process_device(out.data_ptr(), out.stride(0), m, audio.data_ptr(), a_stride, stream)
            bs_.collect_rds(stream=stream)

        try:
            visits = []
            for _ in range(args.visits):
                v = {}
                if bd is not None:
                    v["direct_ms"] = round(timed(direct, args.steps, args.warmup), 3)
                v["split_ms"] = round(timed(behind_split, args.steps, args.warmup), 3)
                visits.append(v)
            entry["visits"] = visits
            s_best = min(v["split_ms"] for v in visits)
            entry["split_stations_real_time"] = round(C * entry["signal_ms_per_call"] / s_best, 1)
            if bd is not None:
                d_best = min(v["direct_ms"] for v in visits)
                entry["direct_stations_real_time"] = round(C * entry["signal_ms_per_call"] / d_best, 1)
                entry["split_over_direct"] = round(d_best / s_best, 3)
        finally:
            res["decode"].append(entry)
            if bd is not None:
                bd.close()
            bs_.close()
            sp.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

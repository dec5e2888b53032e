"""What the polyphase channeliser costs and what it buys (fmd_chan_*, include/fmd.h).

tools/split_bench.py's two geometries: 32 captures x 262 144 samples at 9.6 MS/s with 40 stations each (N 96, D 44,
K 352), and 16 x 524 288 at 19.2 MS/s with 80 stations each (N 192, D 88, K 704).

(a) The channeliser alone, float and s16 input: ms per call and the fraction of its byte floor -- input once plus
    the rows once -- that it reaches at the HBM rate given by --hbm-gbps.
(b) The same captures and stations decoded two ways on one stream: CHANNELISER, the rows handed to a FMD_IN_CIQ_F32
    call of a batch at the rows' rate (2.4 MS/s / 11: no IF stage runs); and SPLITTER, the band splitter plus a batch
    at 2.4 MS/s with a capture map, whose IF stage runs per station.  Reported: ms per call and the stations decoded in
    real time per GPU.  The input is noise: no time of either path depends on what the samples hold.

Device events around `--steps` (alone: `--alone-steps`) back-to-back calls after `--warmup` untimed ones; the two
formats of (a) and the two ways of (b) alternate `--visits` times and every visit is reported.  Prints one JSON line
and writes it to --out.

    python tools/chan_bench.py --out profiles/chan.json

--real and --rows s16 measure the real-sampled form and the int16 rows instead: (c) the real
channeliser (fmd_chan_create_real) against the complex one fed the same samples with a zero Q, at both geometries, and
one real geometry above 256 bins (51.2 MS/s, N 512, D 235), which has no complex form; (d) int16 rows against complex64
rows, the channeliser alone and with the FMD_IN_CIQ_* batch behind it.  Visits alternate as above.

    python tools/chan_bench.py --real --rows s16 --out profiles/chan_real.json
"""
import argparse
import ctypes as C
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
from tools.split_bench import D_BAND, FS_BAND, GEOMETRIES, STATIONS_PER_BAND, T_BAND, band_shifts, timed  # noqa: E402


REAL_BIG = (51.2e6, 512, 235, 4, 1048576, 200)  # fs (real), N, D, captures, samples, rows per capture: the FM band


def _geometries(scale):
    """split_bench's two geometries as (fs, N, D, captures, samples, one capture's station shifts)"""
    for R, G, n, B in GEOMETRIES:
        T, shifts = band_shifts(R, B)
        in_band = [int(2 * s - STATIONS_PER_BAND + 1) for s in range(STATIONS_PER_BAND)]
        yield FS_BAND * R, T, D_BAND * R, max(1, G // scale), n, [bs + k for bs in shifts for k in in_band]


def bench_real(chan, args, stream):
    """--real: the real channeliser against the complex one fed the same samples with a zero Q, visits alternated; and
    one real geometry above 256 bins, which has no complex form."""
    out = []
    cases = [g + (True,) for g in _geometries(args.scale)]
    fs, N, D, G, n, B = REAL_BIG
    cases.append((fs, N, D, max(1, G // args.scale), n, [int(k) for k in range(-B // 2, B - B // 2)], False))
    for fs, N, D, G, n, shifts, twin in cases:
        torch.manual_seed(1)
        v = (0.1 * torch.randn((G, n), dtype=torch.float32, device="cuda")).contiguous()
        S = G * len(shifts)
        real = chan.Channeliser(fs, N, D, G, [shifts] * G, real=True)
        rows = torch.empty((S, real.out_stride(n)), dtype=torch.complex64, device="cuda")
        ways = [("real", real, v)]
        if twin:
            zq = torch.stack([v, torch.zeros_like(v)], dim=2).reshape(G, 2 * n).contiguous()
            ways.append(("complex_zero_q", chan.Channeliser(fs, N, D, G, [shifts] * G), zq))
        ms = {name: [] for name, _, _ in ways}
        for _ in range(args.visits):
            for name, ch, t in ways:
                ms[name].append(round(timed(lambda: ch.process(t, n, out=rows, stream=stream), args.alone_steps,
                                            args.warmup), 4))
        entry = {"fs": fs, "n_bins": N, "decimation": D, "filter_order": 8 * D, "captures": G, "samples": n,
                 "rows": S, "ms_per_call": ms, "input_bytes": {"real": G * n * 4, "complex_zero_q": G * n * 8}}
        if twin:
            entry["complex_over_real"] = round(min(ms["complex_zero_q"]) / min(ms["real"]), 3)
        out.append(entry)
        for _, ch, _ in ways:
            ch.close()
    return out


def bench_rows_s16(pkg, chan, args, stream):
    """--rows s16: int16 rows against complex64 rows, the channeliser alone and with the FMD_IN_CIQ_* batch behind it
    on one stream, visits alternated."""
    out = []
    for fs, N, D, G, n, shifts in _geometries(args.scale):
        torch.manual_seed(1)
        f32 = (0.1 * torch.randn((G, 2 * n), dtype=torch.float32, device="cuda")).contiguous()
        S = G * len(shifts)
        ch = chan.Channeliser(fs, N, D, G, [shifts] * G)
        rows = {"f32": torch.empty((S, ch.out_stride(n)), dtype=torch.complex64, device="cuda"),
                "s16": torch.empty((S, ch.out_stride(n, np.int16), 2), dtype=torch.int16, device="cuda")}
        fmt = {"f32": None, "s16": np.int16}
        params = pkg.make_params(FS_BAND, 0.0, 48000.0, 15000.0, D_BAND, table_size=T_BAND)
        tuning = np.array([int(2 * s - STATIONS_PER_BAND + 1) for s in range(STATIONS_PER_BAND)] *
                          (S // STATIONS_PER_BAND), np.int32)
        batch = pkg.Batch(params, S, tuning_shifts=tuning, record_callbacks=False)
        a_stride = (batch.max_audio_floats(n * int(round(FS_BAND)) // int(round(fs))) + 63) // 64 * 64
        audio = torch.empty((S, a_stride), dtype=torch.float32, device="cuda")
        cnt = C.c_uint()
        a_rows = pkg.make_rows(audio.data_ptr(), pkg.FMD_PCM_F32, a_stride, cnt)

        def alone(k):
            return lambda: ch.process(f32, n, out=rows[k], rows=fmt[k], stream=stream)

        def decode(k):
            def call():
                _, m = ch.process(f32, n, out=rows[k], rows=fmt[k], stream=stream)
                batch.process_call(ciq_in=rows[k][:, :m], audio=a_rows, stream=stream)
                batch.collect_rds(stream=stream)
            return call

        ms = {"alone": {"f32": [], "s16": []}, "decode": {"f32": [], "s16": []}}
        try:
            for _ in range(args.visits):
                for k in ("f32", "s16"):
                    ms["alone"][k].append(round(timed(alone(k), args.alone_steps, args.warmup), 4))
            for _ in range(args.visits):
                for k in ("f32", "s16"):
                    ms["decode"][k].append(round(timed(decode(k), args.steps, args.warmup), 3))
        finally:
            out.append({"fs": fs, "n_bins": N, "decimation": D, "captures": G, "samples": n, "rows": S,
                        "row_bytes": {"f32": S * (n // D) * 8, "s16": S * (n // D) * 4}, "ms_per_call": ms})
            batch.close()
            ch.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--real", action="store_true",
                    help="measure the real channeliser against the zero-Q complex one instead (and N 512)")
    ap.add_argument("--rows", choices=["f32", "s16"], default="f32",
                    help="s16: measure int16 rows against complex64 rows instead, alone and with the batch behind")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--alone-steps", type=int, default=200, help="calls of the channeliser alone per timed window")
    ap.add_argument("--visits", type=int, default=2)
    ap.add_argument("--scale", type=int, default=1, help="divide captures by this (a rehearsal at a small size)")
    ap.add_argument("--hbm-gbps", type=float, default=6290.0,
                    help="the HBM rate the byte floor is taken at (a float4 copy on an MI355X measures 6.29 TB/s)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("chan_bench: no GPU (nothing here is measured on a CPU)")
    pkg = load_package()
    split = import_module(pkg.__name__ + ".split")
    chan = import_module(pkg.__name__ + ".chan")
    stream = torch.cuda.current_stream().cuda_stream
    res = {"steps": args.steps, "alone_steps": args.alone_steps, "warmup": args.warmup, "visits": args.visits,
           "hbm_gbps": args.hbm_gbps, "device": torch.cuda.get_device_name(0), "alone": [], "decode": []}
    if args.real or args.rows == "s16":
        del res["alone"], res["decode"]
        if args.real:
            res["real"] = bench_real(chan, args, stream)
        if args.rows == "s16":
            res["rows_s16"] = bench_rows_s16(pkg, chan, args, stream)
        line = json.dumps(res)
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
    for R, G, n, B in GEOMETRIES:
        G = max(1, G // args.scale)
        fs = FS_BAND * R
        T, shifts = band_shifts(R, B)            # T = the bins of the 100 kHz raster
        N, D = T, D_BAND * R
        per_cap = B * STATIONS_PER_BAND
        S = G * per_cap
        in_band = [int(2 * s - STATIONS_PER_BAND + 1) for s in range(STATIONS_PER_BAND)]
        station_shifts = [bs + k for bs in shifts for k in in_band]      # one capture's stations, as split_bench's
        torch.manual_seed(1)
        f32 = (0.1 * torch.randn((G, 2 * n), dtype=torch.float32, device="cuda")).contiguous()
        s16 = torch.clamp(f32 * 32767.0, -32768, 32767).to(torch.int16).contiguous()
        ch = chan.Channeliser(fs, N, D, G, [station_shifts] * G)
        rows = torch.empty((S, ch.out_stride(n)), dtype=torch.complex64, device="cuda")
        # (a) alone
        alone = {"f32": [], "s16": []}
        for _ in range(args.visits):
            for name, t in (("f32", f32), ("s16", s16)):
                alone[name].append(timed(lambda: ch.process(t, n, out=rows, stream=stream), args.alone_steps,
                                         args.warmup))
        for name, esz in (("f32", 8), ("s16", 4)):
            floor = G * n * esz + S * (n // D) * 8
            floor_ms = floor / (args.hbm_gbps * 1e6)
            res["alone"].append({"fs": fs, "n_bins": N, "decimation": D, "filter_order": 8 * D, "captures": G,
                                 "samples": n, "rows": S, "input": name,
                                 "ms_per_call": [round(v, 4) for v in alone[name]], "floor_bytes": int(floor),
                                 "floor_ms": round(floor_ms, 4),
                                 "fraction_of_floor": round(floor_ms / min(alone[name]), 4),
                                 "gflop_bins": round(8.0 * N * S * (n // D) / 1e9, 2)})
        # (b) the same stations behind the channeliser and behind the splitter
        sp = split.Splitter(fs, R, G, [shifts] * G, table_size=T)
        bands = torch.empty((G * B, sp.out_stride(n)), dtype=torch.complex64, device="cuda")
        params = pkg.make_params(FS_BAND, 0.0, 48000.0, 15000.0, D_BAND, table_size=T_BAND)
        split_shifts = np.array([in_band] * (G * B), np.int32).reshape(-1)
        b_split = pkg.Batch(params, S, tuning_shifts=split_shifts, record_callbacks=False)
        b_split.set_capture_map(np.arange(S, dtype=np.uint32) // STATIONS_PER_BAND, G * B)
        b_chan = pkg.Batch(params, S, tuning_shifts=split_shifts, record_callbacks=False)
        a_stride = (b_split.max_audio_floats(n // R) + 63) // 64 * 64
        audio = torch.empty((S, a_stride), dtype=torch.float32, device="cuda")
        cnt = C.c_uint()
        a_rows = pkg.make_rows(audio.data_ptr(), pkg.FMD_PCM_F32, a_stride, cnt)

        def behind_chan():
            _, m = ch.process(f32, n, out=rows, stream=stream)
            b_chan.process_call(ciq_in=rows[:, :m], audio=a_rows, stream=stream)
            b_chan.collect_rds(stream=stream)

        def behind_split():
            _, m = sp.process(f32, n, out=bands, stream=stream)
            b_split.process_device(bands.data_ptr(), bands.stride(0), m, audio.data_ptr(), a_stride, stream)
            b_split.collect_rds(stream=stream)

        entry = {"R": R, "fs": fs, "captures": G, "samples": n, "stations": S, "bands": B,
                 "signal_ms_per_call": round(n / fs * 1e3, 3)}
        try:
            visits = []
            for _ in range(args.visits):
                visits.append({"chan_ms": round(timed(behind_chan, args.steps, args.warmup), 3),
                               "split_ms": round(timed(behind_split, args.steps, args.warmup), 3)})
            entry["visits"] = visits
            c_best, s_best = min(v["chan_ms"] for v in visits), min(v["split_ms"] for v in visits)
            entry["chan_stations_real_time"] = round(S * entry["signal_ms_per_call"] / c_best, 1)
            entry["split_stations_real_time"] = round(S * entry["signal_ms_per_call"] / s_best, 1)
            entry["split_over_chan"] = round(s_best / c_best, 3)
        finally:
            res["decode"].append(entry)
            b_chan.close()
            b_split.close()
            sp.close()
            ch.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

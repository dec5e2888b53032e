"""Rate of the band scan's spectral pass (fmd_scan_accumulate_device) at 8192 captures x 65 536 samples, float and
byte input, nfft 256 / 1024 / 4096, against the decode-every-step way of the seek test (a batch of G x 24 channels
on shared captures, tests/test_gpu_configs.py::test_seek_stops_on_the_next_stereo_station).  Device events around
`--steps` back-to-back calls after `--warmup` untimed ones.  Prints one JSON line.

    python tools/scan_bench.py --steps 50 --warmup 5
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

FS, D, PEAK = 2.4e6, 11, 8.0e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captures", type=int, default=8192)
    ap.add_argument("--samples", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--decode-steps", type=int, default=10)
    args = ap.parse_args()
    pkg = load_package()
    scan = import_module(pkg.__name__ + ".scan")
    G, n = args.captures, args.samples
    torch.manual_seed(1)
    f32 = (0.1 * torch.randn((G, n, 2), dtype=torch.float32, device="cuda")).contiguous()
    u8 = torch.randint(0, 256, (G, n, 2), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    res = {"captures": G, "samples": n, "steps": args.steps}
    for nfft in (256, 1024, 4096):
        s = scan.Scan(FS, G, nfft=nfft)
        for name, t, u in (("f32", f32, False), ("u8", u8, True)):
            ms = timed(lambda: s.accumulate_device(t.data_ptr(), n, n, stream=stream, u8=u), args.steps, args.warmup)
            nbytes = t.numel() * t.element_size()
            res["%s_n%d_ms" % (name, nfft)] = round(ms, 4)
            res["%s_n%d_GBps" % (name, nfft)] = round(nbytes / ms / 1e6, 1)
            res["%s_n%d_peak_frac" % (name, nfft)] = round(nbytes / ms / 1e-3 / PEAK, 3)
        s.close()
    # the seek test's way: every capture decoded at all 24 tuner steps, 24 channels per capture.  A batch's
    # sub-batches of 8192 channels need a multiple of 24 channels per capture: timed at 341 captures (8184
    # channels, one sub-batch) and scaled to G by the capture count (a batch's time grows with its channels)
    T = 24
    Gd = min(G, 8192 // T)
    b = pkg.Batch(pkg.make_params(FS, 0.0, 48000.0, 15000.0, D, table_size=T), Gd * T,
                  tuning_shifts=np.tile(np.arange(T, dtype=np.int32) - T // 2, Gd), record_callbacks=False)
    b.set_channels_per_capture(T)
    a_stride = (b.max_audio_floats(n) + 63) // 64 * 64
    audio = torch.empty((Gd * T, a_stride), dtype=torch.float32, device="cuda")

    def decode():
        b.process_device(f32.data_ptr(), n, n, audio.data_ptr(), a_stride, stream)
        b.collect_rds(stream=stream)

    try:
        ms = timed(decode, args.decode_steps, 2)
        res["decode_every_step_captures"] = Gd
        res["decode_every_step_ms"] = round(ms, 3)
        res["decode_every_step_ms_scaled_to_G"] = round(ms * G / Gd, 2)
        res["decode_over_scan_f32_n1024"] = round(ms * G / Gd / res["f32_n1024_ms"], 1)
    finally:
        b.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Scalar quantisation on the device (csrc/quantize.hip) next to the numpy path on the same data in the same run.
Float data is drawn on the device with torch.  Per step: HIP-event time, warm-up first, median of --runs runs; bytes moved
(translate: 4 B read + 1 B written per coordinate; parameters: 4 B read per coordinate and pass; normalize: 4 B + 4 B) over time as
a fraction of the 8 TB/s HBM peak.  The numpy functions (quantize.normalize_rows / mips_i8_max_val / mips_i8_translate /
euclid_u8_params / euclid_u8_translate) are timed once each with the wall clock: they take seconds.
usage: quantize_time.py [--n 1000000] [--runs 7] [--big] [--no-numpy] [--out profiles/quantize_time.json]
  --big: also 10M x 200 MIPS on device pointers only (8 GB of floats; no host copy, no numpy leg)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from parlayann_amd import DeviceIndex, _capi, quantize  # noqa: E402

PEAK = 8.0e12
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--big", action="store_true")
ap.add_argument("--no-numpy", action="store_true")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "quantize_time.json"))
args = ap.parse_args()
lib = _capi.load()


def timed(fn, runs=args.runs):
    """median HIP-event milliseconds of fn() on torch's current stream (the handle runs on it too), after two warm-up calls"""
    fn(); fn()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def step(name, ms, nbytes):
    return {"step": name, "ms": round(ms, 4), "GB_moved": round(nbytes / 1e9, 3), "frac_of_8TBps": round(nbytes / (ms * 1e-3) / PEAK, 3)}


def wall(fn):
    t0 = time.perf_counter(); r = fn(); return r, (time.perf_counter() - t0) * 1e3


def draw(n, d, scale):
    g = torch.Generator(device="cuda"); g.manual_seed(1234)
    return torch.randn((n, d), generator=g, device="cuda", dtype=torch.float32) * scale


def params_dev(t, kind, trim=True):
    p = _capi.QuantParams()
    _capi.check(lib.pann_quantize_params_dev(C.c_void_p(t.data_ptr()), t.shape[0], t.shape[1], t.shape[1] * 4, kind, 1 if trim else 0,
                                             C.byref(p), None))
    return p


def rows_dev(t, p, out, normalize_first=False):
    _capi.check(lib.pann_quantize_rows_dev(C.byref(p), C.c_void_p(t.data_ptr()), t.shape[0], t.shape[1] * 4, 1 if normalize_first else 0,
                                           C.c_void_p(out.data_ptr()), t.shape[1], None))


def run_case(n, d, kind, numpy_leg, handle_leg=True):
    mips = kind == "mips_i8"
    k = _capi.PANN_QUANT_MIPS_I8 if mips else _capi.PANN_QUANT_EUCLID_U8
    t = draw(n, d, 0.3 if mips else 1.0)
    if not mips:
        t = t * 3.0 - 0.7
    out = torch.empty((n, d), dtype=torch.uint8, device="cuda")
    nd = n * d
    res = {"n": n, "d": d, "kind": kind, "device": [], "numpy": []}
    dev = res["device"]
    passes = 3 if mips else 1
    if handle_leg:
        X = t.cpu().numpy()
        ix = DeviceIndex(X, max_degree=1, metric="mips" if mips else "Euclidian")
        ix.set_stream(0)                                  # torch's current stream: the events bracket the handle's kernels
        if mips:
            dev.append(step("normalize (in place, index slab)", timed(ix.normalize), nd * 8))
        dev.append(step(f"parameters ({passes} pass{'es' if passes > 1 else ''}, index slab)", timed(lambda: ix.quantize_params(kind, True)), nd * 4 * passes))
        p = ix.quantize_params(kind, True)
        holder = []

        def make():
            for h in holder:
                h.close()
            holder[:] = [ix.quantized(kind, params=p, copy_graph=False)[0]]
        dev.append(step("create_quantized (alloc + clear + translate)", timed(make), nd * 5))
        (q, _), e2e = wall(lambda: ix.quantized(kind, trim=True, copy_graph=False))
        res["device_end_to_end_ms"] = round(e2e + (dev[0]["ms"] if mips else 0.0), 3)      # normalize + parameters + create
        q.close(); [h.close() for h in holder]
        tn = torch.from_numpy(ix.points()).cuda() if mips else t
        ix.close()
    else:
        tn = t
        p = params_dev(tn, k, True)
    dev.append(step(f"parameters ({passes} pass{'es' if passes > 1 else ''}, dense rows)", timed(lambda: params_dev(tn, k, True)), nd * 4 * passes))
    dev.append(step("translate (dense rows)", timed(lambda: rows_dev(tn, p, out)), nd * 5))
    if mips:
        dev.append(step("normalize + translate fused (const rows)", timed(lambda: rows_dev(t, p, out, True)), nd * 5))
    if numpy_leg and handle_leg:
        npl = res["numpy"]
        if mips:
            Xn, ms = wall(lambda: quantize.normalize_rows(X)); npl.append({"step": "normalize_rows", "ms": round(ms, 1)})
            mv, ms = wall(lambda: quantize.mips_i8_max_val(Xn, trim=True)); npl.append({"step": "mips_i8_max_val(trim=True)", "ms": round(ms, 1)})
            _, ms = wall(lambda: quantize.mips_i8_translate(Xn, mv)); npl.append({"step": "mips_i8_translate", "ms": round(ms, 1)})
            res["max_val_equal"] = bool(np.float32(mv) == np.float32(p.max_val))
        else:
            pe, ms = wall(lambda: quantize.euclid_u8_params(X)); npl.append({"step": "euclid_u8_params", "ms": round(ms, 1)})
            _, ms = wall(lambda: quantize.euclid_u8_translate(X, pe)); npl.append({"step": "euclid_u8_translate", "ms": round(ms, 1)})
            res["params_equal"] = bool(pe.slope == np.float32(p.slope) and int(pe.offset) == p.offset)
        res["numpy_end_to_end_ms"] = round(sum(s["ms"] for s in npl), 1)
    print(json.dumps(res), flush=True)
    return res


cases = [run_case(args.n, 200, "mips_i8", not args.no_numpy), run_case(args.n, 96, "euclid_u8", not args.no_numpy)]
if args.big:
    cases.append(run_case(10_000_000, 200, "mips_i8", False, handle_leg=False))
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump({"tool": "tools/quantize_time.py", "runs": args.runs, "device": torch.cuda.get_device_name(0), "cases": cases}, f, indent=1)
    f.write("\n")

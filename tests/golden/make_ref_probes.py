#!/usr/bin/env python3
"""Scalar probes of the UNMODIFIED reference (oracle/_ref/libgenrich_ref.so: the reference with main renamed, built by
oracle/Makefile): calcPval, pchisq, and the fraction codec (addFrac / subFrac / updateVal), on fixed inputs.
Run in the build container only:  python tests/golden/make_ref_probes.py

Commits DATA only: tests/golden/ref_probes.npz, the inputs and what the reference returned for them.
tests/test_oracle.py holds the oracle to these values bit for bit.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libgenrich_ref.so")
OUT = os.path.join(HERE, "ref_probes.npz")
sys.path.insert(0, os.path.dirname(HERE))
import backends as B  # noqa: E402

COUNTS = [2, 3, 4, 5, 6, 8, 10]
TRIALS, STEPS = 300, 40


def load_ref():
    lib = C.CDLL(REF_SO)
    lib.calcPval.restype = C.c_float
    lib.calcPval.argtypes = [C.c_float, C.c_float]
    lib.pchisq.restype = C.c_double
    lib.pchisq.argtypes = [C.c_double, C.c_int]
    lib.updateVal.restype = C.c_float
    lib.updateVal.argtypes = [C.c_int16, C.c_uint8, C.POINTER(C.c_int32), C.POINTER(C.c_uint8)]
    lib.addFrac.argtypes = [C.POINTER(C.c_int16), C.POINTER(C.c_uint8), C.c_uint8]
    lib.subFrac.argtypes = [C.POINTER(C.c_int16), C.POINTER(C.c_uint8), C.c_uint8]
    return lib


def calc_pval(ref):
    rng = np.random.default_rng(5)
    expt = np.concatenate([rng.integers(0, 3000, 4000) / 120.0 * rng.integers(1, 121, 4000),
                           rng.random(2000) * 50, [0, 1, 7, 7.0000005, 1e6, 3e38]]).astype(np.float32)
    ctrl = np.concatenate([rng.random(4000) * 30, rng.random(2000) * 8,
                           [0, -1, 7, 7.0000005, 1e-30, 6.9999995]]).astype(np.float32)
    out = np.array([ref.calcPval(float(e), float(c)) for e, c in zip(expt, ctrl)], dtype=np.float32)
    return dict(pval_expt=expt, pval_ctrl=ctrl, pval_ref=out)


def pchisq(ref):
    rng = np.random.default_rng(6)
    xs, dfs = np.zeros(5000), np.zeros(5000, dtype=np.int32)
    for i in range(5000):
        df = int(rng.integers(2, 201)) * 2
        xs[i] = float(rng.random() * (3 * df if rng.random() < 0.8 else 0.9))
        dfs[i] = df
    out = np.array([ref.pchisq(float(x), int(df)) for x, df in zip(xs, dfs)], dtype=np.float64)
    return dict(chisq_x=xs, chisq_df=dfs, chisq_ref=out)


def fraction_codec(ref, oracle):
    """Per trial: a running pileup seeded with an integer value (run_v, 1/120 units), then STEPS additions / subtractions of
    1/c on one difference element; after each, the element's (cov, frac) state.  At the end the element goes through
    updateVal on the running state: its float, where the total is one the reference accepts (>= 0)."""
    rng = np.random.default_rng(7)
    run_v = np.zeros(TRIALS, dtype=np.int64)
    cnt = np.zeros((TRIALS, STEPS), dtype=np.uint8)
    add = np.zeros((TRIALS, STEPS), dtype=bool)
    cov_s = np.zeros((TRIALS, STEPS), dtype=np.int16)
    frac_s = np.zeros((TRIALS, STEPS), dtype=np.uint8)
    got = np.full(TRIALS, np.nan, dtype=np.float32)
    for t in range(TRIALS):
        cov, frac = C.c_int16(0), C.c_uint8(0)
        rcov, rfrac = C.c_int32(0), C.c_uint8(0)
        v = 0
        run_v[t] = int(rng.integers(0, 5)) * 120 * 50
        ref.updateVal(C.c_int16(int(run_v[t]) // 120), C.c_uint8(0), C.byref(rcov), C.byref(rfrac))
        for s in range(STEPS):
            c = COUNTS[rng.integers(0, len(COUNTS))]
            cnt[t, s] = c
            if rng.random() < 0.5:
                ref.addFrac(C.byref(cov), C.byref(frac), c)
                add[t, s] = True
                v += 120 // c
            else:
                ref.subFrac(C.byref(cov), C.byref(frac), c)
                v -= 120 // c
            cov_s[t, s], frac_s[t, s] = cov.value, frac.value
        # the reference exit()s on a negative canonical integer part (ERRPILE), which a random +/- sequence can reach even
        # for a non-negative total: probed only when the total is >= 0 and the oracle's state is not negative
        neg = C.c_int(0)
        oracle.gxo_getval(int(run_v[t]) + v, C.byref(neg))
        if run_v[t] + v >= 0 and not neg.value:
            got[t] = ref.updateVal(cov, frac, C.byref(rcov), C.byref(rfrac))
    return dict(codec_run_v=run_v, codec_count=cnt, codec_add=add, codec_cov=cov_s, codec_frac=frac_s, codec_ref=got)


def main():
    ref = load_ref()
    out = {}
    out.update(calc_pval(ref))
    out.update(pchisq(ref))
    out.update(fraction_codec(ref, B.Oracle.lib()))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

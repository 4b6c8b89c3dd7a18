"""Pins the CPU oracle (oracle/genrich_oracle.c) to the reference:
 * byte-identical narrowPeak / -f / -k text on every committed golden fixture (the fixtures
   are the unmodified reference's own outputs, tests/golden/make_golden.py);
 * the calcPval known answers printed in the reference's README (README.md:243-249);
 * scalar functions and the fraction codec against what the compiled reference returned
   for the same inputs (tests/golden/ref_probes.npz, tests/golden/make_ref_probes.py).
"""
import ctypes as C
import os

import numpy as np
import pytest

import backends as B
import golden_cases as G


@pytest.mark.parametrize("name", G.case_names())
def test_oracle_matches_reference_outputs(name, tmp_path):
    meta, case, params, names = G.load_case(name)
    o = B.Oracle(params)
    o.set_chroms(case["lens"], case["skip"], case["beds"])
    pile = str(tmp_path / "pile")
    lams, facs = [], []
    for r, (rep, rm) in enumerate(zip(case["replicates"], meta["replicates"])):
        o.sample_begin(0, rep["save"])
        o.push_events(rep["treat"])
        o.sample_end()
        if rep["ctrl"] is not None:
            o.sample_begin(1, None)
            o.push_events(rep["ctrl"])
            _, lam, fac = o.sample_end()
            facs.append(fac)
        else:
            lam = o.sample_no_control()
        lams.append(lam)
        cname = None if rm["control"] is None else (
            "null" if rm["control"] == "null" else meta["tmp_prefix"] + rm["ctrl_name"])
        o.pvalues_to(pile, r > 0, names, meta["tmp_prefix"] + rm["expt_name"], cname)
    peaks_opt = "-X" not in meta["args"]
    npk, glen, bp = o.find_peaks_to(str(tmp_path / "np"), str(tmp_path / "log"), names, peaks_opt)

    assert [f"{v:f}" for v in lams] == [f"{v:f}" for v in meta["ref_lambda"]]
    assert [f"{v:f}" for v in facs] == [f"{v:f}" for v in meta["ref_factor"]]
    assert glen == meta["ref_genome_len"][0]
    assert open(pile, "rb").read() == G.read_gz(name, "out.pile")
    assert open(tmp_path / "log", "rb").read() == G.read_gz(name, "out.log")
    if peaks_opt:
        assert [npk, bp] == meta["ref_peaks"][0]
        assert open(tmp_path / "np", "rb").read() == G.read_gz(name, "out.narrowPeak")
        if name not in ("nopeaks_log",):
            assert npk > 0, "fixture should exercise the peak sweep"


def test_calc_pval_readme_known_answers():
    """README.md:243-249: seven -f rows of a real hg19 run, control 2.477916."""
    lib = B.Oracle.lib()
    kat = {33: 3.183460, 34: 3.231466, 35: 3.278469, 36: 3.324516,
           39: 3.457329, 40: 3.499948, 41: 3.541798}
    for e, want in kat.items():
        got = lib.gxo_calc_pval(float(e), 2.477916)
        assert abs(got - want) <= 1.5e-6, (e, got, want)


def test_calc_pval_special_values():
    """calcPval's early exits (Genrich.c:1629-1634) and SURVEY Appendix B probes."""
    lib = B.Oracle.lib()
    fmax = float(np.finfo(np.float32).max)
    assert lib.gxo_calc_pval(5.0, -1.0) == -1.0
    assert lib.gxo_calc_pval(0.0, 0.0) == 0.0
    assert lib.gxo_calc_pval(1.0, 0.0) == fmax
    assert lib.gxo_calc_pval(0.0, 3.0) == 0.0
    assert abs(lib.gxo_calc_pval(30.0, 10.0) - 1.38409615) < 1e-6
    assert abs(lib.gxo_calc_pval(5.0, 10.0) - 0.179538146) < 1e-7
    assert abs(lib.gxo_calc_pval(1e6, 1.0) - 51.0932045) < 1e-5
    assert abs(lib.gxo_pchisq(2 * 7 / np.log10(np.e), 4) - 5.76654455) < 1e-7
    assert abs(lib.gxo_pchisq(2 * 0.6 / np.log10(np.e), 6) - 0.076787925) < 1e-8


def test_getval_fraction_text():
    """pileup floats of thirds print as the reference's."""
    lib = B.Oracle.lib()
    neg = C.c_int(0)
    assert f"{lib.gxo_getval(40, C.byref(neg)):f}" == "0.333333"
    assert f"{lib.gxo_getval(160, C.byref(neg)):f}" == "1.333333"
    assert f"{lib.gxo_getval(1160, C.byref(neg)):f}" == "9.666667"
    assert lib.gxo_getval(120 * 77, C.byref(neg)) == 77.0 and not neg.value


# ---- scalar probes of the compiled reference ------------------------------------------
# tests/golden/ref_probes.npz: fixed inputs and what oracle/_ref/libgenrich_ref.so (the unmodified reference, main renamed)
# returned for them, recorded by tests/golden/make_ref_probes.py.

def _probes():
    return np.load(os.path.join(G.GOLDEN, "ref_probes.npz"))


def test_calc_pval_bitexact_vs_reference():
    d, lib = _probes(), B.Oracle.lib()
    assert len(d["pval_ref"]) == 6006
    for e, c, a in zip(d["pval_expt"], d["pval_ctrl"], d["pval_ref"]):
        b = lib.gxo_calc_pval(float(e), float(c))
        assert np.float32(a).tobytes() == np.float32(b).tobytes(), (e, c, a, b)


def test_pchisq_bitexact_vs_reference():
    d, lib = _probes(), B.Oracle.lib()
    assert len(d["chisq_ref"]) == 5000
    for x, df, a in zip(d["chisq_x"], d["chisq_df"], d["chisq_ref"]):
        b = lib.gxo_pchisq(float(x), int(df))
        assert a == b or (np.isnan(a) and np.isnan(b)), (x, df, a, b)


def test_fraction_codec_is_exact_rational():
    """The (cov, frac) state of the reference after any add/sub sequence, and the running
    state of updateVal, are pure functions of the exact sum in 1/120 units."""
    d, lib = _probes(), B.Oracle.lib()
    neg = C.c_int(0)
    probed = 0
    assert d["codec_cov"].shape == (300, 40)
    for t in range(d["codec_cov"].shape[0]):
        v = 0
        run_v = int(d["codec_run_v"][t])
        for s in range(d["codec_cov"].shape[1]):
            c = int(d["codec_count"][t, s])
            v += 120 // c if d["codec_add"][t, s] else -(120 // c)
            cov, frac = int(d["codec_cov"][t, s]), int(d["codec_frac"][t, s])
            # element value must equal v/120 exactly:  cov + e/8 + s/6 + t/10
            e, sx, tn = frac & 7, (frac >> 3) & 3, (frac >> 5) & 7
            assert sx < 3 and tn < 5
            assert 120 * cov + 15 * e + 20 * sx + 12 * tn == v
            assert (cov == 0 and frac == 0) == (v == 0)
        # the reference exit()s on a negative canonical integer part (ERRPILE, 1921/1969), which a
        # random +/- sequence can reach even for a non-negative total: probed only when it is >= 0
        want = lib.gxo_getval(run_v + v, C.byref(neg))
        got = d["codec_ref"][t]
        if run_v + v >= 0 and not neg.value:
            assert np.float32(got).tobytes() == np.float32(want).tobytes()
            probed += 1
        else:
            assert np.isnan(got)
    assert probed > 200

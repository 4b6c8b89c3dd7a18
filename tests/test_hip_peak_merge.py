"""peak_N names the same peak in every file of a run, however the chromosomes lie on the contexts: the six group writers with a row
(or a group of rows) per called peak -- narrowPeak, --counts, --peak-signal, --summits, --gc-peaks, --motif-hits -- over three
contexts that own interleaved chromosomes ({0, 3}, {1}, {2}) write the bytes one context writes, and their tables name the same
peaks (genrich_amd/csrc/gx_peak_merge.h; the merge itself, without a device: tests/test_peak_merge.py)."""
import ctypes as C
import os
import re
import threading

import pytest

import backends as B
import motifs_ref as MR
from genrich_amd import synth
from genrich_amd.lib import _to_tmpfile, gc_peaks_text, load_library, motif_hits_text
from ranks import ThreadAllreduce
from test_hip_gcbias import _push_whole, _seqs

pytestmark = pytest.mark.gpu

LENS = [400_000, 300_000, 350_000, 250_000]
NAMES = ["chrA", "chrB", "chrC", "chrD"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "motifs_small.jaspar")


def _run(seqs, motifs, ev, owned=None, coll=None):
    import genrich_amd
    h = genrich_amd.Genrich(B.make_params(pq=0.01, min_auc=20.0))
    h.set_chroms(LENS, None)
    if owned is not None:
        h.set_owned(owned)
    if coll:
        h.set_collectives(*coll)
    h.set_genome(True)
    h.set_genome_bases(True)
    _push_whole(h, seqs)
    h.set_motifs(motifs)
    h.set_count_in_peaks(True)
    h.sample_begin(0, None)
    h.push_events(ev)
    h.sample_end()
    h.sample_no_control()
    h.pvalues()
    h.find_peaks()
    return h


def _files(hs, motifs, ids, mnames, pthr):
    """The six tables over the contexts hs, by their group writers."""
    lib = load_library()
    arr = (C.c_void_p * len(hs))(*[h.ctx for h in hs])
    nm = (C.c_char_p * len(NAMES))(*[n.encode() for n in NAMES])
    smp = (C.c_char_p * 1)(b"treatment")
    for h in hs:
        assert h.count_in_peaks() == 1
    chk = hs[0]._check
    return {
        "narrowPeak": _to_tmpfile(lambda f: chk(lib.gx_write_narrowpeak_group(arr, len(hs), nm, f))),
        "counts": _to_tmpfile(lambda f: chk(lib.gx_write_counts_group(arr, len(hs), nm, 1, smp, f))),
        "peak-signal": _to_tmpfile(lambda f: chk(lib.gx_write_peak_signal_group(arr, len(hs), nm, f))),
        "summits": _to_tmpfile(lambda f: chk(lib.gx_write_summits_group(arr, len(hs), nm, 25, 50, f))),
        "gc-peaks": gc_peaks_text(hs, NAMES),
        "motif-hits": motif_hits_text(hs, NAMES, motifs, ids, mnames, pthr),
    }


def test_three_contexts_with_interleaved_chromosomes_number_the_peaks_alike_in_all_six_files():
    seqs = _seqs(41, LENS)
    motifs, ids, mnames, pthr = [], [], [], []
    for mid, mname, counts in MR.read_jaspar(open(GOLDEN, "rb").read()):
        s = MR.pssm(counts, 1.0)
        t, _, _, n_ge, un = MR.threshold(s, 0.01)
        motifs.append((s, t))
        ids.append(mid)
        mnames.append(mname)
        pthr.append(float("nan") if un else MR.p_achieved(n_ge, len(s)))
    ev = synth.make_fragments(LENS, 300_000, 64, peak_every=20_000, tower_every=3_000_000)
    one = _run(seqs, motifs, ev)
    want = _files([one], motifs, ids, mnames, pthr)

    owns, coll = [[1, 0, 0, 1], [0, 1, 0, 0], [0, 0, 1, 0]], ThreadAllreduce(3)
    hs, errors = [None] * 3, []

    def rank(r):
        try:
            hs[r] = _run(seqs, motifs, ev, owned=owns[r], coll=(r, 3, coll.callback(r)))
        except BaseException as e:
            errors.append(e)
            coll.bar.abort()

    threads = [threading.Thread(target=rank, args=(r,)) for r in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    pks = [h.get_peaks() for h in hs]                                 # (the contexts stay open until the writers have run)
    assert sorted(set(pks[0]["chrom"].tolist())) == [0, 3] and set(pks[1]["chrom"].tolist()) == {1} and set(pks[2]["chrom"].tolist()) == {2}
    assert sum(len(p) for p in pks) == one.n_peaks
    for c in range(4):
        assert int((one.get_peaks()["chrom"] == c).sum()) > 5
    got = _files(hs, motifs, ids, mnames, pthr)
    for h in hs + [one]:
        h.close()

    for name in want:
        assert got[name] == want[name], name

    def rows(name, header):
        lines = got[name].decode().splitlines()[header:]
        assert lines
        return [l.split("\t") for l in lines]

    # the four tables with a row per peak: the same rows chr, start, end, peak_N, numbered from 0 in chromosome order
    peak_rows = [r[:4] for r in rows("narrowPeak", 0)]
    assert [r[3] for r in peak_rows] == ["peak_%d" % i for i in range(len(peak_rows))] and len(peak_rows) == sum(len(p) for p in pks)
    assert [NAMES.index(r[0]) for r in peak_rows] == sorted(NAMES.index(r[0]) for r in peak_rows)
    for name in ("counts", "peak-signal", "gc-peaks"):
        assert [r[:4] for r in rows(name, 1)] == peak_rows, name
    # the two with rows inside peaks: every peak_N they name is that row of the narrowPeak, with its coordinates
    by_name = {r[3]: r for r in peak_rows}
    summit_rows, hit_rows = rows("summits", 1), rows("motif-hits", 1)
    assert len(summit_rows) >= len(peak_rows) and len(hit_rows) > 20
    for r in summit_rows:                                              # chr start end peak_N.j ... peak_start peak_end
        pk = by_name[re.fullmatch(r"(peak_\d+)\.\d+", r[3]).group(1)]
        assert [r[0], r[9], r[10]] == pk[:3] and int(pk[1]) <= int(r[1]) < int(pk[2])
    for r in hit_rows:                                                 # chr start end ID score strand NAME peak_N ...
        pk = by_name[r[7]]
        assert r[0] == pk[0] and int(pk[1]) <= int(r[1]) and int(r[2]) <= int(pk[2])
    assert {r[0] for r in hit_rows} == set(NAMES) and {r[0] for r in summit_rows} == set(NAMES)

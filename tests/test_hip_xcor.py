"""Strand cross-correlation of each sample's 5' ends on the GPU (gx_set_xcor / gx_push_tags, genrich-amd --xcor): the two kernels
alone through gx_xcor_tags, real samples, two contexts and the command line, against tests/xcor_ref.py.

The reference counts n11(d) once per set of tags over the widest range (-4096, 4096); a narrower range is a slice of it (n11(d)
does not depend on the range).  Every comparison is == on integers, or on bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import backends as B
import golden_cases as G
import xcor_ref as R
from genrich_amd import synth
from genrich_amd.lib import GX_PATH_XCOR, TAG_DTYPE, XCOR_MIN_TILE, xcor_geometry, xcor_group, xcor_text
from test_hip_complexity import ACTIVE6, OWNED6, SAVE6, SKIP6
from test_hip_counts import _cli_inputs
from test_host_cli import _binary

pytestmark = pytest.mark.gpu

ORDER = -10
LENS8 = [1, 63, 64, 65, 127, 128, 5000, 200_000]
RANGES = [(-100, 600), (0, 0), (64, 64), (-1, 63), (-4096, 4096)]
WIDE = (-4096, 4096)
# six chromosomes under test_hip_complexity's masks: 3 is skipped (-e), 4 is outside the sample's save mask, 5 is not owned
LENS6 = [300_000, 200_003, 70_001, 50_000, 50_000, 50_000]


def _tags(rows):
    a = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    t = np.zeros(len(a), dtype=TAG_DTYPE)
    t["chrom"], t["pos"], t["strand"] = a[:, 0], a[:, 1], a[:, 2]
    return t


def _rows(t):
    return np.stack([t["chrom"], t["pos"], t["strand"]], 1).astype(np.int64)


def _random_tags(lens, density, seed, strands=(0, 1)):
    rng = np.random.default_rng(seed)
    parts = []
    for c, L in enumerate(lens):
        for s in strands:
            pos = np.nonzero(rng.random(L) < density)[0]
            parts.append(np.stack([np.full(len(pos), c), pos, np.full(len(pos), s)], 1))
    return _tags(np.concatenate(parts))


def _ctx(lens=LENS8, skip=None, owned=None):
    import genrich_amd
    h = genrich_amd.Genrich(B.make_params(pq=0.01, min_auc=20.0))
    h.set_chroms(lens, skip)
    if owned is not None:
        h.set_owned(owned)
    return h


def _counts(x):
    return R.Counts(x.n_pos, x.n_plus, x.n_minus, x.rejected, x.lo, x.hi, x.n11)


@pytest.fixture(scope="module")
def hook():
    h = _ctx()
    yield h
    h.close()


@pytest.fixture(scope="module")
def sets():
    """{name: (lens, tags, the reference's counts over the widest range)}, made once."""
    full = [(c, x, s) for c in (5,) for x in range(128) for s in (0, 1)]
    out = {"half": (LENS8, _random_tags(LENS8, 0.5, 1)), "sparse": (LENS8, _random_tags(LENS8, 0.01, 2)),
           "one_full": (LENS8, np.concatenate([_random_tags(LENS8[:5] + [0, 5000, 200_000], 0.05, 3), _tags(full)])),
           "no_minus": (LENS8, np.concatenate([_random_tags(LENS8[:7] + [0], 0.1, 4), _random_tags([0] * 7 + [200_000], 0.1, 5, strands=(1,))]))}
    out = {k: (lens, t, R.counts(lens, _rows(t), *WIDE)) for k, (lens, t) in out.items()}
    assert out["one_full"][2].n11[4096] >= 128 and out["half"][2].n_plus > 100_000 > out["sparse"][2].n_plus > 1000
    assert all(c.rejected == 0 and c.n_pos == sum(LENS8) for _, _, c in out.values())
    return out


# ---- 1: the hook against the reference ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["half", "sparse", "one_full", "no_minus"])
def test_the_hook_against_the_reference(hook, sets, name):
    lens, tags, wide = sets[name]
    for lo, hi in RANGES:
        got = hook.xcor_tags(lens, tags, lo, hi)
        assert _counts(got) == R.sub_range(wide, lo, hi), (name, lo, hi)
    assert hook.path_info() & GX_PATH_XCOR


# ---- 2: chromosome borders ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mirrored", [False, True])
def test_pairs_never_cross_a_chromosome_border(hook, mirrored):
    lens = [5000, 130, 70, 5000]
    for a, b in ((0, 1), (1, 2), (2, 3)):
        sa, sb = (0, 1) if mirrored else (1, 0)
        rows = [(a, x, sa) for x in range(max(0, lens[a] - 70), lens[a])] + [(b, x, sb) for x in range(min(70, lens[b]))]
        for lo, hi in RANGES:
            got = hook.xcor_tags(lens, _tags(rows), lo, hi)
            assert got.n11 == [0] * (hi - lo + 1) and got.n_plus + got.n_minus == len(rows) and got.rejected == 0, (a, b, lo, hi)


# ---- 3: tile and halo -----------------------------------------------------------------------------------------------------------

def test_partners_in_the_next_tiles_and_before_the_tile(hook):
    tile = XCOR_MIN_TILE
    bits = 64 * tile
    lens = [40 * bits]
    pad_bits = 64 * xcor_geometry()[3]               # (the chromosome starts `pad` words into the vector: tile t begins at bit t * bits - pad_bits of it)
    dists = (1, 63, 64, 65, 4096)
    rows = []
    for t in (3, 4, 11, 20):                         # the last word of tile t, every bit of it taken in turn
        last = t * bits - pad_bits + bits - 64
        for k, d in enumerate(dists):
            for bit in (0, 1 + k, 63):
                x = last + bit
                rows += [(0, x, 1), (0, x + d, 0)]          # the partner in the next tile, or (4096) a tile further
                y = t * bits - pad_bits + bit + 7 * k       # ... and plus tags in the first word of a tile with partners before it
                rows += [(0, y, 1), (0, y - d, 0)]
    tags = _tags(rows)
    wide = R.counts(lens, _rows(tags), *WIDE)
    for d in dists:
        assert wide.n11[4096 + d] >= 12 and wide.n11[4096 - d] >= 12
    for lo, hi in RANGES + [(-4096, -4000), (4090, 4096)]:
        for tw in (tile, 0):
            assert _counts(hook.xcor_tags(lens, tags, lo, hi, 0, tw)) == R.sub_range(wide, lo, hi), (lo, hi, tw)


# ---- 4: order, split, repeats (the hook, and real pushes) -------------------------------------------------------------------------

def test_order_split_and_repeats(hook, sets):
    lens, tags, wide = sets["sparse"]
    exp = R.sub_range(wide, -100, 600)
    rng = np.random.default_rng(9)
    shuffled = tags[rng.permutation(len(tags))]
    tripled = np.repeat(shuffled, 3)
    assert _counts(hook.xcor_tags(lens, shuffled, -100, 600)) == exp
    got = hook.xcor_tags(lens, tripled, -100, 600)
    assert _counts(got) == exp and got.n_plus + got.n_minus == len(tags)          # positions, not tags
    h = _ctx()
    h.set_xcor(-100, 600)
    ev = synth.make_fragments([lens[7]], 2000, 3)
    ev["chrom"] = 7
    for rep, (src, step) in enumerate(((tags[:300], 1), (shuffled, 7), (tripled, 100_000))):
        h.sample_begin(0, None)
        h.push_events(ev)
        for at in range(0, len(src), step):
            h.push_tags(src[at:at + step])
        h.sample_end()
        h.sample_no_control()
        h.pvalues()
    assert h.xcor_samples() == 3
    assert _counts(h.xcor(0)) == R.counts(lens, _rows(tags[:300]), -100, 600)
    assert _counts(h.xcor(1)) == exp == _counts(h.xcor(2)) and [h.xcor(k).rep for k in range(3)] == [0, 1, 2]
    h.close()


# ---- 5: launch geometry ---------------------------------------------------------------------------------------------------------

def test_every_launch_geometry_gives_the_same_integers(hook, sets):
    lanes, grid0, tile0, pad, flush = xcor_geometry()
    lens, tags, wide = sets["half"]
    for lo, hi in ((-100, 600), (-4096, 4096)):
        exp = R.sub_range(wide, lo, hi)
        for grid in (1, 2, 0):
            for tw in (XCOR_MIN_TILE, 192, tile0):
                assert _counts(hook.xcor_tags(lens, tags, lo, hi, grid, tw)) == exp, (lo, hi, grid, tw)
    lib, ctx = hook.lib, hook.ctx
    ln, t = np.asarray(lens, dtype=np.uint32), tags
    for grid, tw, word in ((1 << 16, 0, "65535"), (0, 32, "multiple of 64"), (0, 100, "multiple of 64"), (0, 2048, "multiple of 64")):
        assert lib.gx_xcor_tags(ctx, ln.ctypes.data, len(ln), t.ctypes.data, len(t), 0, 10, grid, tw, None, None, None, None, None, 0) == ORDER
        assert word in lib.gx_last_error(ctx).decode()
    for lo, hi in ((-4097, 0), (0, 4097), (5, 4)):
        assert lib.gx_xcor_tags(ctx, ln.ctypes.data, len(ln), t.ctypes.data, len(t), lo, hi, 0, 0, None, None, None, None, None, 0) == ORDER
        assert "-4096 <= lo <= hi <= 4096" in lib.gx_last_error(ctx).decode()


# ---- 6: rejected tags -----------------------------------------------------------------------------------------------------------

def test_rejected_tags_are_counted_and_change_nothing_else(hook, sets):
    lens, tags, wide = sets["sparse"]
    bad = _tags([(len(lens), 0, 1), (len(lens) + 5, 10, 0), (0xFFFFFFFF, 0, 1), (0, 1, 1), (1, 63, 0), (7, 200_000, 1), (7, 0xFFFFFFFF, 0), (6, 10, 2)])
    mixed = np.concatenate([tags[:1000], bad, tags[1000:]])
    exp = R.sub_range(wide, -100, 600)._replace(rejected=len(bad))
    assert R.counts(lens, _rows(mixed), -100, 600) == exp
    assert _counts(hook.xcor_tags(lens, mixed, -100, 600)) == exp
    got = hook.xcor_tags(lens, bad, 0, 5)
    assert (got.n_plus, got.n_minus, got.rejected, got.n11) == (0, 0, len(bad), [0] * 6)
    assert _counts(hook.xcor_tags(lens, tags[:0], 0, 5)) == R.Counts(sum(lens), 0, 0, 0, 0, 5, [0] * 6)


# ---- 7: real samples ------------------------------------------------------------------------------------------------------------

def _planted6(seed, dist):
    """Tags on all six chromosomes of LENS6 (three take part): plus tags with partners `dist` further, and background."""
    rng = np.random.default_rng(seed)
    rows = []
    for c, L in enumerate(LENS6):
        xs = rng.integers(0, L - 700, 3000)                        # (with repeats: a position tagged twice is tagged once)
        rows += [np.stack([np.full(3000, c), xs, np.ones(3000, dtype=np.int64)], 1), np.stack([np.full(3000, c), xs + dist, np.zeros(3000, dtype=np.int64)], 1),
                 np.stack([np.full(500, c), rng.integers(0, L, 500), rng.integers(0, 2, 500)], 1)]
    return _tags(np.concatenate(rows))


def test_real_samples_keep_their_own_bits():
    h = _ctx(LENS6, SKIP6, OWNED6)
    assert not h.path_info() & GX_PATH_XCOR
    h.set_xcor(-100, 600)
    h.set_knob("GX_XCOR_TILE", 192)
    ev = synth.make_fragments(LENS6[:3], 20_000, 5)
    tags = [_planted6(11, 180), _planted6(12, 75), _planted6(13, 300)]
    for is_ctrl, save, t in ((0, SAVE6, tags[0]), (1, None, tags[1])):
        h.sample_begin(is_ctrl, save)
        h.push_events(ev)
        h.push_tags(t[:5000])
        h.push_tags(t[5000:])
        h.sample_end()
    h.pvalues()
    h.set_knob("GX_XCOR_GRID", 1)
    h.set_knob("GX_XCOR_TILE", 0)
    h.sample_begin(0, SAVE6)
    h.push_events(ev)
    h.push_tags(tags[2])
    h.sample_end()
    assert h.xcor_samples() == 3 and h.path_info() & GX_PATH_XCOR
    exp = [R.counts(LENS6, _rows(t), -100, 600, ACTIVE6) for t in tags]
    got = [h.xcor(k) for k in range(3)]
    assert [_counts(g) for g in got] == exp and [(g.rep, g.is_ctrl) for g in got] == [(0, False), (0, True), (1, False)]
    assert [int(np.argmax(e.n11)) - 100 for e in exp] == [180, 75, 300] and exp[0].n_pos == sum(LENS6[:3])
    assert exp[0].n11[280] > 8000 > 1000 > exp[1].n11[280] and exp[1].n11[175] > 8000 > 1000 > exp[2].n11[175]     # no sample sees another's bits
    assert [h.xcor(k) for k in range(3)] == got                  # asked twice
    curve, met = xcor_text([h], 36)
    samples = [(g.rep, g.is_ctrl, e) for g, e in zip(got, exp)]
    assert curve.decode() == R.curve_text(samples) and met.decode() == R.metrics_text(samples, 36)
    h.reset()
    assert h.xcor_samples() == 0 and not h.path_info() & GX_PATH_XCOR
    assert h.lib.gx_get_xcor(h.ctx, 0, *([None] * 9), 0) == ORDER
    h.sample_begin(0, SAVE6)                                      # the setting stays
    h.push_tags(tags[1])
    h.push_events(ev)
    h.sample_end()
    assert _counts(h.xcor(0)) == exp[1]
    h.close()


# ---- 8: two contexts ------------------------------------------------------------------------------------------------------------

def test_two_contexts_add_up():
    lens = LENS6[:3]
    tags = _planted6(21, 150)
    tags = tags[tags["chrom"] < 3]
    ev = synth.make_fragments(lens, 20_000, 6)
    whole = R.counts(lens, _rows(tags), -50, 400)
    hs = []
    for owned in ([1, 0, 1], [0, 1, 0], [1, 1, 1]):
        h = _ctx(lens, None, owned)
        h.set_xcor(-50, 400)
        h.sample_begin(0, None)
        h.push_events(ev)
        h.push_tags(tags)
        h.sample_end()
        assert _counts(h.xcor(0)) == R.counts(lens, _rows(tags), -50, 400, owned)
        hs.append(h)
    got = xcor_group(hs[:2], 0)
    assert _counts(got) == whole == _counts(hs[2].xcor(0)) and (got.rep, got.is_ctrl) == (0, False)
    assert xcor_text(hs[:2], 50) == xcor_text(hs[2:], 50)
    fresh = _ctx(lens)                                            # a context without a result
    assert hs[0].lib.gx_xcor_group((C.c_void_p * 2)(hs[0].ctx, fresh.ctx), 2, 0, *([None] * 9), 0) == ORDER
    for h in hs + [fresh]:
        h.close()


# ---- 11: option off, and the order rules ----------------------------------------------------------------------------------------

def test_option_off_and_the_order_rules():
    import genrich_amd
    h = genrich_amd.Genrich(B.make_params(pq=0.01, min_auc=20.0))
    lib, ctx = h.lib, h.ctx
    assert lib.gx_set_xcor(ctx, -100, 600) == ORDER              # before gx_set_chroms
    h.set_chroms([100_000])
    t = _tags([(0, 5, 1), (0, 50, 0)])
    ev = synth.make_fragments([100_000], 2000, 3)
    h.sample_begin(0, None)
    assert lib.gx_push_tags(ctx, t.ctypes.data, 2) == ORDER      # the option is off
    assert lib.gx_set_xcor(ctx, -100, 600) == ORDER              # a sample is open
    h.push_events(ev)
    h.sample_end()
    assert h.xcor_samples() == 0 and not h.path_info() & GX_PATH_XCOR
    assert lib.gx_set_xcor(ctx, -100, 600) == ORDER              # after the first sample
    h.reset()
    for lo, hi in ((-4097, 0), (0, 4097)):
        assert lib.gx_set_xcor(ctx, lo, hi) == ORDER and "-4096 <= lo <= hi <= 4096" in lib.gx_last_error(ctx).decode()
    h.set_xcor(0, 60)
    assert lib.gx_push_tags(ctx, t.ctypes.data, 2) == ORDER      # no sample open
    h.sample_begin(0, None)
    h.push_tags(t)
    h.push_events(ev)
    h.sample_end()
    assert h.xcor(0).n11[45] == 1 and sum(h.xcor(0).n11) == 1
    h.reset()
    h.set_xcor(0, -1)                                             # off again
    h.sample_begin(0, None)
    assert lib.gx_push_tags(ctx, t.ctypes.data, 2) == ORDER
    h.push_events(ev)
    h.sample_end()
    assert h.xcor_samples() == 0 and not h.path_info() & GX_PATH_XCOR
    h.close()


# ---- 9: the command line, single-end ----------------------------------------------------------------------------------------------

def _single_end_sam(path):
    """A few thousand single-end reads of length 36, one alignment each, unique names: plus reads at x and minus reads whose last
    base is x + 179, over two chromosomes, and unrelated background.  Returns the tags the reads give."""
    rng = np.random.default_rng(17)
    lens = [300_000, 120_000]
    lines = ["@HD\tVN:1.0\tSO:queryname\n"] + [f"@SQ\tSN:chr{c + 1}\tLN:{L}\n" for c, L in enumerate(lens)]
    rows, k = [], 0

    def read(c, first, plus):
        nonlocal k
        lines.append(f"r{k}\t{0 if plus else 16}\tchr{c + 1}\t{first + 1}\t30\t36M\t*\t0\t0\t*\t*\tAS:i:0\n")
        rows.append((c, first if plus else first + 35, 1 if plus else 0))
        k += 1
    for c, L in enumerate(lens):
        for x in rng.integers(100, L - 1000, 1500):
            read(c, int(x), True)
            read(c, int(x) + 179 - 35, False)
        for x in rng.integers(0, L - 36, 600):
            read(c, int(x), bool(rng.integers(0, 2)))
    with open(path, "w") as f:
        f.write("".join(lines))
    return lens, np.asarray(rows, dtype=np.int64)


def test_cli_single_end_reads(tmp_path):
    sam = str(tmp_path / "se.sam")
    lens, rows = _single_end_sam(sam)
    c = R.counts(lens, rows, -100, 600)
    samples = [(0, False, c)]
    assert R.metrics(c, 36)["fragment_length"] == 180 and c.rejected == 0
    exp = (R.curve_text(samples), R.metrics_text(samples, 36))
    for tag, extra in (("one", []), ("two", ["--devices", "0,0"])):     # one context; two contexts on one GPU: the same bytes
        out = str(tmp_path / tag)
        res = subprocess.run([_binary(), "-v", "-y", "-X", "-t", sam, "--xcor", out + ".tsv", "--xcor-metrics", out + ".met", "--xcor-read-length", "36"]
                             + extra, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        assert (open(out + ".tsv").read(), open(out + ".met").read()) == exp
        assert "suggested -x 180" in res.stderr and "fragment length 180" in res.stderr
    # an extension chosen: nothing is suggested; the tags are those of the reads, not of the extended intervals
    out = str(tmp_path / "w")
    res = subprocess.run([_binary(), "-v", "-w", "150", "-X", "-t", sam, "--xcor-metrics", out + ".met", "--xcor-read-length", "36"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert open(out + ".met").read() == exp[1] and "suggested" not in res.stderr and not os.path.exists(out + ".tsv")
    # other shifts, no read length, gzip
    import gzip
    res = subprocess.run([_binary(), "-z", "-y", "-X", "-t", sam, "--xcor", out + ".tsv", "--xcor-shifts", "150,200"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert gzip.open(out + ".tsv.gz", "rb").read().decode() == R.curve_text([(0, False, R.sub_range(c, 150, 200))])


# ---- 10: the command line, paired fixtures ----------------------------------------------------------------------------------------

def _fixture_samples(name):
    """[(rep, is_ctrl, Counts)] of a fixture whose -b lines are all whole proper-pair fragments, from its events.bed alone: + at
    the start and - at the end - 1 of every line."""
    meta, case, params, names = G.load_case(name)
    assert not {"-j", "-y", "-w", "-x"} & set(meta["args"])
    lens = case["lens"]
    per = {}
    for line in G.read_gz(name, "events.bed").decode().splitlines():
        ch, s, e, nm = line.split("\t")
        _, cnt, kind, smp = nm.rsplit("_", 3)
        ci, s, e = names.index(ch), int(s), int(e)
        assert 0 <= s < e <= lens[ci], line                      # (that no end was clamped to the length: the run's -v warnings, below)
        per.setdefault((int(smp), kind == "C"), []).extend([(ci, s, 1), (ci, e - 1, 0)])
    out = []
    for r, rep in enumerate(case["replicates"]):
        active = [sv and not sk for sv, sk in zip(rep["save"], case["skip"])]     # (a chromosome the treatment file does not name takes no part)
        for ctrl in ([False, True] if rep["ctrl"] is not None else [False]):
            out.append((r, ctrl, R.counts(lens, np.asarray(per.get((r, ctrl), []), dtype=np.int64).reshape(-1, 3), -100, 600, active)))
    return out, meta


@pytest.mark.parametrize("name", ["ctrl_q", "dups_pairs", "reps3_p_missing", "bedx"])
def test_cli_paired_fixtures(name):
    samples, meta = _fixture_samples(name)
    assert all(c.n_plus > 100 and c.rejected == 0 for _, _, c in samples)
    _, args, tmp, _ = _cli_inputs(name)
    runs = [("xc", args)]
    if "-r" in args:       # a PCR duplicate of a pair has the pair's two ends: the bits, and so the curve, are the same without -r
        runs.append(("xc_nor", [a for a in args if a != "-r"]))
    for tag, a in runs:
        out = os.path.join(tmp, tag + "_out")
        res = subprocess.run([_binary(), "-v", "-o", out + ".narrowPeak", "--xcor", out + ".tsv"] + a, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        assert "prevented from extending" not in res.stderr       # no -b line was clamped: every interval is a whole fragment
        assert open(out + ".tsv").read() == R.curve_text(samples), tag
        if tag == "xc" and "-X" not in meta["args"]:
            assert open(out + ".narrowPeak", "rb").read() == G.read_gz(name, "out.narrowPeak")
    out = os.path.join(tmp, "xcu_out")
    res = subprocess.run([_binary(), "-o", out + ".narrowPeak", "--xcor", out + ".tsv", "--xcor-unpaired"] + args, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    rows = [l.split("\t") for l in open(out + ".tsv").read().splitlines()[1:] if not l.startswith("#")]
    assert len(rows) == 701 * len(samples) and all(r[2] == "0" and r[3] == "NA" for r in rows)

"""Several ranks in one process: one context per thread, every exchange of the library (gx_set_collectives) through a
barrier-and-sum callback -- the way the command line runs its contexts (--devices).  One GPU process, no spawn, no gloo: an N-rank
run of a tiny input costs little more than the N contexts.  Used by test_hip_bh_ranks.py and test_hip_peak_signal.py."""
import os
import threading

import numpy as np

import backends as B
from genrich_amd.dist import lpt_partition
from genrich_amd.lib import GX_IV_FINAL

MAX_WORLD = 8            # contexts side by side in one process: no test goes beyond


class ThreadAllreduce:
    """gx_set_collectives' sum over contexts that run side by side in threads of this process, as the command line's do.
    A rank that fails aborts the barrier (run_ranks does, on any exception): the others' callbacks then return 1 and the
    library returns an error to them -- nobody is left waiting; a rank that never arrives ends the wait after `timeout` s."""

    def __init__(self, world, timeout=120):
        self.bar = threading.Barrier(world, timeout=timeout)
        self.bufs = [None] * world

    def callback(self, rank):
        def cb(buf, n, _user):
            try:
                a = np.ctypeslib.as_array(buf, shape=(n,))
                self.bufs[rank] = a.copy()
                self.bar.wait()
                total = np.sum(self.bufs, axis=0)
                self.bar.wait()                     # (everyone has read every buffer)
                a[:] = total
                return 0
            except Exception as e:                  # (never across the C boundary)
                print("allreduce callback failed:", e)
                return 1
        return cb


class RankResult:
    """What one rank of run_ranks came back with."""

    def __init__(self, rank, owned, scal, peaks, flags, iv, n_iv):
        self.rank, self.owned, self.scal, self.peaks, self.flags, self.iv, self.n_iv = rank, owned, scal, peaks, flags, iv, n_iv


def _drive(be, reps, sel=lambda ev: ev):
    """sample_begin .. find_peaks on one backend -> [(fragLen, lambda, factor)] per replicate (factor 1 without a control)"""
    scal = []
    for tr, ct in reps:
        be.sample_begin(0, None)
        be.push_events(sel(tr))
        frag, _, _ = be.sample_end()
        if ct is not None:
            be.sample_begin(1, None)
            be.push_events(sel(ct))
            _, lam, fac = be.sample_end()
        else:
            lam, fac = be.sample_no_control(), 1.0
        be.pvalues()
        scal.append((frag, lam, fac))
    be.find_peaks()
    return scal


def _intervals(be, chroms):
    """{chromosome: (ends, p, q)} of the final array"""
    out = {}
    for c in chroms:
        end, cols = be.get_intervals(GX_IV_FINAL, c)
        out[c] = (end, cols["p"], cols["q"])
    return out


def run_oracle(params, lens, reps, skip=None, beds=None):
    """One backends.Oracle run of the whole genome -> a RankResult (rank 0 of 1) that also keeps the treatment pileups:
    .expt[c], next to .iv[c] = (ends, p, q)"""
    o = B.Oracle(params)
    try:
        o.set_chroms(lens, skip, beds)
        scal = _drive(o, reps)
        peaks = o.get_peaks()
        res = RankResult(0, np.ones(len(lens), dtype=np.uint8), scal, peaks, 0, {}, 0)
        res.expt = {}
        for c in range(len(lens)):
            end, cols = o.get_intervals(GX_IV_FINAL, c)
            res.iv[c] = (end, cols["p"], cols["q"])
            res.expt[c] = cols["expt"]
            res.n_iv += len(end)
        return res
    finally:
        o.close()


_POOL = {"key": None, "ctxs": []}   # the contexts of the last run, kept for the next: up to MAX_WORLD, whatever the world sizes


def close_pool():
    for h in _POOL["ctxs"]:
        if h is not None:
            h.close()
    _POOL["key"], _POOL["ctxs"] = None, []


def _pool(key):
    """The kept contexts for `key` = (the parameters' bytes, the environment they were made in): others are closed first, so
    that no more than MAX_WORLD are ever open."""
    if _POOL["key"] != key:
        close_pool()
        _POOL["key"], _POOL["ctxs"] = key, [None] * MAX_WORLD
    return _POOL["ctxs"]


def run_ranks(params, lens, reps, world, owner=None, skip=None, beds=None, knobs=None, env=None, wrap=None, timeout=30, fresh=False):
    """`world` contexts, one thread each, over the chromosomes of `owner` (default: genrich_amd.dist.lpt_partition; a rank it
    leaves without a chromosome gets an all-zero mask): set_chroms, set_owned, set_collectives, then every replicate of
    reps = [(treatment, control | None)] with the rank's own chromosomes' events only, pvalues, find_peaks.
    knobs: {name: value} for gx_set_knob on every context; env: {name: value} in the environment while the contexts are made
    (the library reads it once, in gx_create); wrap(rank, callback) -> callback: a rank's all-reduce as the test wants it.
    Eight contexts take most of a second to make (profiles/r23_bh_ranks.txt), so a run leaves its contexts behind and the next
    run with the same parameters and environment takes them again after gx_reset (rank r: the r-th, whatever the world
    sizes); fresh=True, or a run with knobs, makes its own and closes them.  A run in which a rank failed closes them all.
    -> [RankResult] by rank.  Every thread is joined whatever happened; the first exception is raised again here."""
    import genrich_amd

    assert 1 <= world <= MAX_WORLD
    owner = list(lpt_partition(lens, world) if owner is None else owner)
    masks = [np.array([o == r for o in owner], dtype=np.uint8) for r in range(world)]
    coll = ThreadAllreduce(world, timeout=timeout)
    key = (bytes(params), tuple(sorted((env or {}).items())))
    fresh = fresh or bool(knobs)
    ctxs = [None] * world if fresh else _pool(key)
    out, errors = [None] * world, []
    lock = threading.Lock()

    def rank(r):
        try:
            if ctxs[r] is None:
                ctxs[r] = genrich_amd.Genrich(params)
            else:
                ctxs[r].reset()
            h = ctxs[r]
            h.set_chroms(lens, skip, beds)
            h.set_owned(masks[r])
            cb = coll.callback(r)
            h.set_collectives(r, world, wrap(r, cb) if wrap else cb)
            for k, v in (knobs or {}).items():
                h.set_knob(k, v)
            scal = _drive(h, reps, lambda ev: ev[masks[r][ev["chrom"]].astype(bool)])
            mine = [c for c in range(len(lens)) if masks[r][c]]
            n_iv = sum(len(h.get_intervals(GX_IV_FINAL, c, piles=False)[0]) for c in range(len(lens)))
            out[r] = RankResult(r, masks[r], scal, h.get_peaks(), h.path_info(), _intervals(h, mine), n_iv)
        except BaseException as e:
            with lock:
                errors.append((r, e))
            coll.bar.abort()

    saved = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update({k: str(v) for k, v in (env or {}).items()})
    threads = [threading.Thread(target=rank, args=(r,)) for r in range(world)]
    try:
        for t in threads:
            t.start()
    finally:
        for t in threads:
            if t.ident is not None:
                t.join()
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        if fresh:
            for h in ctxs:
                if h is not None:
                    h.close()
        elif errors or any(o is None for o in out):
            close_pool()
    if errors:
        run_ranks.last_errors = sorted(errors, key=lambda x: x[0])
        # (the rank that failed first, not one that the broken barrier sent home)
        first = [e for _, e in errors if "allreduce callback failed" not in str(e)] or [errors[0][1]]
        raise first[0]
    return out


def assert_equals_oracle(res, ora, lens):
    """The ranks of one run against the single-process oracle, in bits: every owned interval's end, p and q, the scalars of
    every replicate on every rank, the merged peak list; every chromosome has exactly one owner, and a rank without one
    returns no peak and no interval."""
    from genrich_amd.dist import merge_peaks

    seen = np.zeros(len(lens), dtype=int)
    for r in res:
        seen += r.owned
        for (f, lam, fac), (fo, lamo, faco) in zip(r.scal, ora.scal):
            assert f == fo, ("fragLen", r.rank, f, fo)
            assert np.float32(lam).tobytes() == np.float32(lamo).tobytes(), ("lambda", r.rank, lam, lamo)
            assert np.float32(fac).tobytes() == np.float32(faco).tobytes(), ("factor", r.rank, fac, faco)
        assert len(r.scal) == len(ora.scal)
        assert sorted(r.iv) == np.flatnonzero(r.owned).tolist()
        for c, (end, p, q) in r.iv.items():
            eo, po, qo = ora.iv[c]
            assert np.array_equal(end, eo), ("ends", r.rank, c)
            assert np.array_equal(p.view(np.uint32), po.view(np.uint32)), ("p", r.rank, c)
            bad = np.flatnonzero(q.view(np.uint32) != qo.view(np.uint32))
            assert len(bad) == 0, ("q", r.rank, c, len(bad), p[bad[:4]], q[bad[:4]], qo[bad[:4]])
        assert r.n_iv == sum(len(r.iv[c][0]) for c in r.iv), ("intervals on chromosomes of other ranks", r.rank, r.n_iv)
        assert set(r.peaks["chrom"].tolist()) <= set(r.iv), r.rank
        if not r.owned.any():
            assert len(r.peaks) == 0 and r.n_iv == 0, r.rank
    assert (seen == 1).all(), seen
    merged = merge_peaks([r.peaks for r in res])
    assert merged.tobytes() == ora.peaks.tobytes(), ("peaks", len(merged), len(ora.peaks))

"""Every route of a peak call runs once.  The host decides a whole gx_find_peaks in one place (plan_call, gx_host_call.h: what
the sweep walks, which replicates are materialised and how, the route of Benjamini-Hochberg, its exchange, its kernels'
instances, where the sweep's masks come from) and the stages read that plan; gx_path_info reports from it.  A route that
the plan mislabels, or an instance table with a wrong row, shows only when a run asks for it -- so each route runs here on
one small input, must give the oracle's bytes (assert_same_run) and must report exactly the path word below.

The words are literals.  They were recorded by running this matrix against the build BEFORE plan_call existed (the
calling half still deciding inline, the path bits still separate flags of the context): the plan has to reproduce every
bit, cross-conditions included.

Sizing.  lens = [200,000, 90,000]: 49 + 22 = 71 tiles of 4,096 bases.  24,000 fragments with a peak every 20,000 bases, -p at
0.01 and -q at 0.1: the smallest round shape at which every route has a peak (with 20,000 fragments -q on one replicate
without a control, and with -E regions, calls none), some hundred distinct p-values and a tile border inside a candidate.

GX_BH_CAPLOG=6 with -q on one replicate without a control is the one case that was NOT recorded before: there the earlier
build took -q on the loose slots, whose k_bh_small inserts up to PV_WHOLE keys with an unbounded probe into a table of 64
slots.  plan_call takes that route only when the table has at least 2 x PV_WHOLE slots; the run must take the tight table,
whose insertions are bounded and grow the table."""
import functools

import pytest

import backends as B
import synth
from test_hip_parity import assert_same_run, hip_backend
from test_hip_paths import PACK_HIST, Q_LOOSE

pytestmark = pytest.mark.gpu

LENS = [200_000, 90_000]
BEDS = [[0, 900, 5_000, 5_001, 12_300, 12_390, 40_000, 60_000, 190_000, 190_070], [500, 600, 60_000, 64_123, 89_000, 90_000]]


@functools.lru_cache(maxsize=None)
def _case(kind):
    tr = synth.make_fragments(LENS, 24_000, 271, peak_every=20_000)
    if kind == "frac":
        tr = synth.add_multimap(tr, LENS, 0.3, 272)
    reps = [dict(save=None, treat=tr, ctrl=None)]
    if kind == "ctrl":
        reps[0]["ctrl"] = synth.make_fragments(LENS, 18_000, 273, uniform_only=True)
    if kind == "reps2":
        reps.append(dict(save=None, treat=synth.make_fragments(LENS, 24_000, 274, peak_every=20_000), ctrl=None))
    case = dict(lens=LENS, replicates=reps)
    if kind == "bed":
        case["beds"] = BEDS
    return case


@functools.lru_cache(maxsize=None)
def _oracle(kind, qval):
    """The oracle's run of a case, made once and shared by the routes that call the same peaks."""
    params = B.make_params(pq=0.1 if qval else 0.01, qval=qval, min_auc=20.0)
    o = B.Oracle(params)
    return params, o, B.run_case(o, _case(kind))


# route -> (case, -q, switches in the environment when the context is made, what follows the first run, expected path word)
ROUTES = {
    "single_p": ("single", False, {}, None, 536870931),
    "single_q": ("single", True, {}, None, 59411),
    "single_q_no_q_loose": ("single", True, {"GX_NO_Q_LOOSE": "1"}, None, 10257),
    "single_q_no_pack_hist": ("single", True, {"GX_NO_PACK_HIST": "1"}, None, 8209),
    "single_q_no_lazy_q": ("single", True, {"GX_NO_LAZY_Q": "1"}, None, 59411),
    "single_q_no_loose": ("single", True, {"GX_NO_LOOSE": "1"}, None, 10257),
    "frac_p": ("frac", False, {}, "learn", 16531),
    "ctrl_p": ("ctrl", False, {}, None, 1041),
    "ctrl_q": ("ctrl", True, {}, None, 9233),
    "ctrl_q_bh0": ("ctrl", True, {"GX_BH_VARIANT": "0"}, None, 9233),
    "ctrl_q_bh1": ("ctrl", True, {"GX_BH_VARIANT": "1"}, None, 9233),
    "ctrl_q_bh2": ("ctrl", True, {"GX_BH_VARIANT": "2"}, None, 9233),
    "ctrl_q_qt_multi": ("ctrl", True, {"GX_QT_MULTI": "1"}, None, 9233),
    "reps2_p": ("reps2", False, {}, None, 17),
    "reps2_q": ("reps2", True, {}, None, 8209),
    "bed_q": ("bed", True, {}, None, 8209),
    "single_p_again": ("single", False, {}, "again", 19),
    "single_q_again": ("single", True, {}, "again", 59411),
    "ctrl_q_again": ("ctrl", True, {}, "again", 9233),
    "single_p_reset": ("single", False, {}, "reset", 536870931),
    "single_q_reset": ("single", True, {}, "reset", 59411),
    "coll_dense": ("single", True, {"GX_FORCE_COLL": "1"}, None, 8241),
    "coll_range": ("single", True, {"GX_FORCE_COLL": "1", "GX_NO_DENSE_BH": "1"}, None, 8273),
}


def run_route(name, setenv):
    """One route on a context of its own -> (oracle, context, the two runs' scalars, the case, the path word).  The word is read
    before anybody asks for intervals, as a caller that only wants the peaks would see it."""
    kind, qval, env, then, _ = ROUTES[name]
    for k, v in env.items():
        setenv(k, v)   # (read when the context is made)
    params, o, so = _oracle(kind, qval)
    case = _case(kind)
    h = hip_backend(params)
    if "GX_FORCE_COLL" in env:
        h.set_collectives(0, 1, lambda buf, n, user: 0)   # (one rank: the sum over all ranks is what is there)
    if kind == "frac":
        h.expect_fractional(True)
    sh = B.run_case(h, case)
    if then == "again":      # a second gx_find_peaks on the same context
        h.find_peaks()
    elif then in ("reset", "learn"):   # (learn: the first run found out that the data holds fractions, the second knows)
        h.reset()
        sh = B.run_case(h, case)
    return o, h, so, sh, case, h.path_info()


@pytest.mark.parametrize("name", list(ROUTES))
def test_every_route_of_a_peak_call_gives_the_oracles_bytes_and_its_path_word(monkeypatch, name):
    o, h, so, sh, case, flags = run_route(name, monkeypatch.setenv)
    assert h.n_peaks > 0
    assert_same_run(o, h, so, sh, case)
    assert flags == ROUTES[name][4], (name, flags, ROUTES[name][4])
    h.close()


def test_q_on_the_loose_slots_is_not_taken_with_a_table_smaller_than_its_keys(monkeypatch):
    """GX_BH_CAPLOG=6: 64 slots cannot take k_bh_small's keys, so the run takes the tight table.  Its histogram's table
    (k_bh_from_dense) is full at once, which raises ST_HASH_FULL: the table grows and is filled by k_bh_hist -- seen from
    outside as PACK_HIST clear on a run that sets it with the default table (single_q_no_q_loose above), and as the oracle's
    q-values from a table that started smaller than the run's distinct p-values."""
    monkeypatch.setenv("GX_BH_CAPLOG", "6")
    params, o, so = _oracle("single", True)
    case = _case("single")
    h = hip_backend(params)
    sh = B.run_case(h, case)
    flags = h.path_info()
    assert h.n_peaks > 0
    assert_same_run(o, h, so, sh, case)
    assert not flags & Q_LOOSE, flags
    assert ROUTES["single_q_no_q_loose"][4] & PACK_HIST and not flags & PACK_HIST, flags
    h.close()

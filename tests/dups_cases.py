"""Inputs for -r (PCR duplicates) made to be CONTESTED: alignment sets with several alignments that share keys with other sets.

The device decides a set of one alignment from "who held this key first" (gx_dups_first); a key that a multi-alignment set also
holds is contested and is walked by the host in the reference's order, on tables that hold the contested keys only (findDups,
genrich_amd/host/host_dups.h).  tests/synth.py's write_sam_dups gives only proper pairs a secondary alignment, and scores
it 3 below the best, so it is dropped unless -s is that large; here secondary alignments carry the primary's AS and survive
without -s."""
import numpy as np

from synth import write_alignment_records

READ_LEN = 50
QUALS = (20, 30, 30, 40)        # per-base qualities, one per mate: few values, so many sets have equal quality sums


def contested_records(names, lens, ev, seed, name_prefix="c", n_hot=120):
    """Queryname-grouped alignment records (write_alignment_records' tuples), deterministic from `seed`, one template per event of
    `ev` (whose fragments give the coordinates; those shorter than a read are left out).  More than half of the templates take
    their coordinates from the first n_hot fragments, so that keys are shared all over:

      pair      a proper pair on a fragment: key (chromosome, both 5' ends)
      pair2     a proper pair with one or two secondary PAIRS of the same AS, sometimes on the primary's own fragment (two alignments
                of one set with one key)
      single    one mate aligned, forward at a fragment's start or reverse at its end -- the very ends a kept pair on that fragment
                puts into the singleton table --, or up to three bases inside: key (chromosome, 5' end, strand)
      single2   one mate with two or three alignments of the same AS, sometimes twice on one end
      dcAxB     both mates aligned, not as a proper pair: A alignments of R1, B of R2 (1x1, 2x1, 1x2, 2x2), every R1 x R2
                combination a key; a third of them repeat an earlier discordant template, half of those with the mates swapped

      plant     three templates that make sure of the case contested keys exist for, in one of the three tables (see plant below)

    A multi-alignment set that matches a kept set through ONE alignment is a duplicate and gives up all its keys: a single-alignment
    set that comes later in quality order and holds one of the other keys must then be kept.  The order is the quality sum's,
    descending and stable, so every set meets sets it shares keys with on both sides."""
    rng = np.random.Generator(np.random.PCG64(seed))
    rl = READ_LEN
    frags = []
    for i in range(len(ev)):
        c, s, e = int(ev["chrom"][i]), int(ev["start"][i]), int(ev["end"][i])
        if e - s >= rl + 10 and e <= lens[c]:
            frags.append((c, s, e))
    hot = frags[:n_hot]

    def pick():
        return hot[int(rng.integers(0, len(hot)))] if rng.random() < 0.6 else frags[int(rng.integers(0, len(frags)))]

    def pick_end():  # (chromosome, pos0, reverse): the forward read at a fragment's start or the reverse read at its end ...
        c, s, e = pick()
        d = int(rng.integers(1, 4)) if rng.random() < 0.4 else 0     # ... or up to three bases inside it: no end of a pair
        return (c, e - rl - d, True) if rng.random() < 0.5 else (c, s + d, False)

    def quals():
        if rng.random() < 0.03:
            return None                          # no qualities: a sum of 0
        return np.full(rl, QUALS[int(rng.integers(0, len(QUALS)))], dtype=np.uint8)

    recs, earlier_dc = [], []

    def emit_pair(nm, alns, q1, q2):
        for k, (c, s, e) in enumerate(alns):
            sec = 256 if k else 0
            recs.append((nm, 99 | sec, c, s, 30, rl, c, e - rl, e - s, -2, None if k else q1))
            recs.append((nm, 147 | sec, c, e - rl, 30, rl, c, s, -(e - s), -3, None if k else q2))

    def emit_single(nm, ends, mate, q):
        for k, (c, p, rev) in enumerate(ends):
            recs.append((nm, 1 | 8 | mate | (16 if rev else 0) | (256 if k else 0), c, p, 30, rl, -1, -1, 0, -1, None if k else q))

    def emit_dc(nm, r1, r2, q1, q2):
        for k in range(max(len(r1), len(r2))):   # the primary records of both mates first, then the secondary ones
            if k < len(r1):
                c, p, rev = r1[k]
                recs.append((nm, 1 | 64 | (16 if rev else 0) | (32 if r2[0][2] else 0) | (256 if k else 0), c, p, 30, rl,
                             r2[0][0], r2[0][1], 0, -1, None if k else q1))
            if k < len(r2):
                c, p, rev = r2[k]
                recs.append((nm, 1 | 128 | (16 if rev else 0) | (32 if r1[0][2] else 0) | (256 if k else 0), c, p, 30, rl,
                             r1[0][0], r1[0][1], 0, -2, None if k else q2))

    def plant(names3):
        """Three templates on coordinates of their own, in any file order: A (best qualities, one alignment) is kept; M (two
        alignments: A's and another, k2) is A's duplicate and gives up k2 as well; S (worst qualities, one alignment, k2) finds k2
        free and is kept -- although the FIRST set that held k2 in the visiting order is M."""
        qa, qm, qs = (np.full(rl, v, dtype=np.uint8) for v in (40, 30, 20))
        table = ("pr", "dc", "sn")[int(rng.integers(0, 3))]
        na, nm_, ns = (names3[k] for k in rng.permutation(3))
        if table == "pr":
            (c1, s1, e1), (c2, s2, e2) = frags[int(rng.integers(0, len(frags)))], frags[int(rng.integers(0, len(frags)))]
            f1, f2 = (c1, s1 + 5, e1 - 5), (c2, s2 + 6, e2 - 4)
            emit_pair(na, [f1], qa, qa)
            emit_pair(nm_, [f2, f1] if rng.random() < 0.5 else [f1, f2], qm, qm)
            emit_pair(ns, [f2], qs, qs)
            return
        def far():                                # (an end seven bases further inside its fragment than any other)
            c, p, rev = pick_end()
            return (c, p - 7, True) if rev else (c, p + 7, False)
        a, a2, b = far(), far(), far()
        if table == "sn":
            mate = 64 if rng.random() < 0.5 else 128
            emit_single(na, [a], mate, qa)
            emit_single(nm_, [a2, a] if rng.random() < 0.5 else [a, a2], 192 - mate if rng.random() < 0.5 else mate, qm)
            emit_single(ns, [a2], mate, qs)
        else:                                     # M: R1 at a or a2, R2 at b; S: M's second combination with the mates swapped
            emit_dc(na, [a], [b], qa, qa)
            emit_dc(nm_, [a2, a], [b], qm, qm)
            emit_dc(ns, [b], [a2], qs, qs)

    kinds = ["pair", "pair2", "single", "single2", "dc1x1", "dc2x1", "dc1x2", "dc2x2", "plant"]
    weight = np.array([0.21, 0.13, 0.19, 0.13, 0.10, 0.07, 0.07, 0.06, 0.04])
    i = 0
    while i < len(frags):
        nm = f"{name_prefix}{i}"
        i += 1
        kind = kinds[int(rng.choice(len(kinds), p=weight))]
        if kind == "plant":
            plant([nm, f"{name_prefix}{i}", f"{name_prefix}{i + 1}"])
            i += 2
        elif kind in ("pair", "pair2"):
            alns = [pick()]
            if kind == "pair2":
                for _ in range(1 if rng.random() < 0.75 else 2):
                    alns.append(alns[0] if rng.random() < 0.15 else pick())
            emit_pair(nm, alns, quals(), quals())
        elif kind in ("single", "single2"):
            ends = [pick_end()]
            if kind == "single2":
                for _ in range(1 if rng.random() < 0.7 else 2):
                    ends.append(ends[0] if rng.random() < 0.15 else pick_end())
            emit_single(nm, ends, 64 if rng.random() < 0.5 else 128, quals())
        else:
            a, b = int(kind[2]), int(kind[4])
            if earlier_dc and rng.random() < 0.35:
                r1, r2 = earlier_dc[int(rng.integers(0, len(earlier_dc)))]
                if rng.random() < 0.5:
                    r1, r2 = r2, r1
                r1, r2 = list(r1[:a]), list(r2[:b])
            else:
                r1, r2 = [], []
            while len(r1) < a:
                r1.append(pick_end())
            while len(r2) < b:
                r2.append(pick_end())
            earlier_dc.append((tuple(r1), tuple(r2)))
            emit_dc(nm, r1, r2, quals(), quals())
    return recs


def write_sam_contested(path, names, lens, ev, seed, name_prefix="c", bam=False):
    write_alignment_records(path, names, lens, contested_records(names, lens, ev, seed, name_prefix), bam=bam)


# ---- the reference's rule on the records themselves (findDups, Genrich.c:3949-4042), for the tests that ask what a case holds ----

def alignment_sets(recs, bam=False):
    """The alignment sets of queryname-grouped records as -r keeps them when every alignment has the best score: per table
    ("pr" proper pairs, "dc" discordant, "sn" singletons) a list of (name, quality sum, keys, ends[, (R1 alignments, R2 alignments)]) in file order.  keys: a pair's
    (chromosome, 5' end of R1, 5' end of R2), a singleton's end (chromosome, 5' end, forward), a discordant combination's two ends
    as a frozenset of (end, how many of the two) -- the table is keyed on the unordered pair.  ends: what a kept set adds to the
    singleton table.  A record without qualities counts 0 in SAM; in BAM its 0xFF bytes sum to -length, which wraps (sumQual)."""
    by_name, order = {}, []
    for r in recs:
        if r[0] not in by_name:
            by_name[r[0]] = []
            order.append(r[0])
        by_name[r[0]].append(r)
    out = dict(pr=[], dc=[], sn=[])
    for nm in order:
        rs = by_name[nm]
        qual = {64: 0, 128: 0}
        for r in rs:
            mate = r[1] & 0xC0
            if not qual[mate]:
                qual[mate] = int(r[10].sum()) if r[10] is not None else ((-r[5]) & 0xFFFF if bam else 0)
        end = lambda r: (r[2], r[3] + r[5] if r[1] & 16 else r[3], not r[1] & 16)
        if any((r[1] & 3) == 3 for r in rs):
            keys, ends = [], []
            for r in rs:
                if r[1] & 64:                    # (R1 forward at s, R2 reverse ending at e = s + tlen)
                    keys.append((r[2], r[3], r[3] + r[8]))
                    ends += [(r[2], r[3], True), (r[2], r[3] + r[8], False)]
            out["pr"].append((nm, min(qual[64] + qual[128], 0xFFFF), keys, ends))
            continue
        r1, r2 = [end(r) for r in rs if r[1] & 64], [end(r) for r in rs if r[1] & 128]
        if r1 and r2:
            keys = [frozenset([(a, 1 + (a == b)), (b, 1 + (a == b))]) for a in r1 for b in r2]
            out["dc"].append((nm, min(qual[64] + qual[128], 0xFFFF), keys, r1 + r2, (len(r1), len(r2))))
        else:
            out["sn"].append((nm, qual[64] if r1 else qual[128], r1 + r2, []))
    return out


def walk(sets, single_opt=True):
    """The reference's decisions: ({name of a duplicate: name of the set it matched}, what the walk met).  The second is a dict of
    counts of the situations a contested case is made for (see test_dups_first.py)."""
    dup_of, seen = {}, dict(multi_sets=dict(pr=0, dc=0, sn=0), shapes=set(), same_key_twice=0, equal_quality=0, single_before_multi=0,
                            single_after_multi=0, kept_after_a_multi_gave_up=dict(pr=0, dc=0, sn=0), sn_on_pair_end=0, sn_on_dc_end=0,
                            sn_on_an_end_a_multi_sn_holds=0, multi_dup=dict(pr=0, dc=0, sn=0))
    tab_sn, sn_from = {}, {}
    for t in ("pr", "dc", "sn"):
        if t != "pr" and not single_opt:
            break
        rows = sets[t]
        ordr = sorted(range(len(rows)), key=lambda i: -rows[i][1])          # (stable)
        quals = [r[1] for r in rows]
        seen["equal_quality"] += sum(1 for q in quals if quals.count(q) > 1)
        multi_keys_pos = {}                                                  # key -> the visiting positions of the multi sets that hold it
        for p, i in enumerate(ordr):
            if len(rows[i][2]) > 1:
                for k in set(rows[i][2]):
                    multi_keys_pos.setdefault(k, []).append(p)
        if t == "sn":
            multi_sn_keys = set(multi_keys_pos)
        tab = tab_sn if t == "sn" else {}
        gave_up = set()                                                      # keys of multi sets that turned out duplicates
        for p, i in enumerate(ordr):
            nm, _, keys, ends = rows[i][:4]
            multi = len(keys) > 1
            if multi:
                seen["multi_sets"][t] += 1
                seen["same_key_twice"] += len(set(keys)) < len(keys)
            if t == "dc":
                seen["shapes"].add(rows[i][4])
            if not multi and keys[0] in multi_keys_pos:
                seen["single_after_multi"] += any(q < p for q in multi_keys_pos[keys[0]])
                seen["single_before_multi"] += any(q > p for q in multi_keys_pos[keys[0]])
            hit = next((k for k in keys if k in tab), None)
            if hit is not None:
                dup_of[nm] = tab[hit]
                if multi:
                    seen["multi_dup"][t] += 1
                    gave_up.update(keys)
                if t == "sn" and hit in sn_from:
                    seen["sn_on_pair_end" if sn_from[hit] == "pr" else "sn_on_dc_end"] += 1
                    seen["sn_on_an_end_a_multi_sn_holds"] += hit in multi_sn_keys
                continue
            if not multi and keys[0] in gave_up:
                seen["kept_after_a_multi_gave_up"][t] += 1
            for k in keys:
                tab.setdefault(k, nm)
            if single_opt:
                for e in ends:
                    if e not in tab_sn:
                        tab_sn[e] = nm
                        sn_from[e] = t
    return dup_of, seen

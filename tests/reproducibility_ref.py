"""--reproducibility's support predicate and figures once more, by brute force over every pair of peaks: what
tests/test_reproducibility.py and tests/test_hip_reproducibility.py hold the library against (include/genrich_amd.h,
gx_peaks_supported, gx_reproducibility_figures).  Python's integers for one pair, int64 for a matrix of pairs: nothing wraps."""
import numpy as np

VERDICTS = ("pass", "borderline", "fail", "NA")


def supports(a, b, pct):
    """Peak b supports peak a: one chromosome, ov >= 1 shared bases and 100 ov >= pct min(len a, len b)."""
    if a["chrom"] != b["chrom"]:
        return False
    ov = min(int(a["end"]), int(b["end"])) - max(int(a["start"]), int(b["start"]))
    shorter = min(int(a["end"]) - int(a["start"]), int(b["end"]) - int(b["start"]))
    return ov >= 1 and 100 * ov >= pct * shorter


def supported(a, b, pct):
    """hit[i]: some peak of b supports a[i]; every pair of peaks on one chromosome is compared (`supports`, as a matrix per
    chromosome in int64: 100 ov stays below 2^39)."""
    hit = np.zeros(len(a), dtype=bool)
    if not len(a) or not len(b):
        return hit.tolist()
    f = lambda x, k: np.asarray(x[k], dtype=np.int64)
    for c in np.intersect1d(a["chrom"], b["chrom"]):
        ia, ib = np.flatnonzero(a["chrom"] == c), np.flatnonzero(b["chrom"] == c)
        sa, ea, sb, eb = f(a, "start")[ia, None], f(a, "end")[ia, None], f(b, "start")[None, ib], f(b, "end")[None, ib]
        ov = np.minimum(ea, eb) - np.maximum(sa, sb)
        shorter = np.minimum(ea - sa, eb - sb)
        hit[ia] = ((ov >= 1) & (100 * ov >= pct * shorter)).any(axis=1)
    return hit.tolist()


def call_index(R, kind, rep=0, half=0):
    """The place of a call in gx_reproducibility's order: "alone" r, "self" r h, "pooled" h."""
    return {"alone": rep, "self": R + 2 * rep + half, "pooled": 3 * R + half}[kind]


def labels(R):
    return ([f"t{r + 1}" for r in range(R)] + [f"t{r + 1}.pr{h + 1}" for r in range(R) for h in range(2)]
            + [f"pooled.pr{h + 1}" for h in range(2)])


def _both(x, y):
    return [p and q for p, q in zip(x, y)]


def figures(run, lists, pct):
    """The figures from the run's peaks and the 3 R + 2 lists in gx_reproducibility's order, as a dict."""
    R = (len(lists) - 2) // 3
    sup = [supported(run, l, pct) for l in lists]
    f = dict(R=R, run_supported=[sum(s) for s in sup], in_run=[sum(supported(l, run, pct)) for l in lists])
    f["nt_pair"], f["best"], f["nt"], cons = [], None, 0, [False] * len(run)
    for i in range(R):
        for j in range(i + 1, R):
            both = _both(sup[i], sup[j])
            f["nt_pair"].append(sum(both))
            if f["best"] is None or sum(both) > f["nt"]:       # (a tie: the first pair)
                f["best"], f["nt"], cons = (i, j), sum(both), both
    pooled = _both(sup[3 * R], sup[3 * R + 1])
    f["np"] = sum(pooled)
    f["n_self"] = [sum(_both(supported(lists[r], lists[R + 2 * r], pct), supported(lists[r], lists[R + 2 * r + 1], pct))) for r in range(R)]
    hi, lo = max(f["np"], f["nt"]), min(f["np"], f["nt"])
    s_hi, s_lo = max(f["n_self"]), min(f["n_self"])
    f["rescue"] = None if R == 1 or lo == 0 else hi / lo
    f["self_consistency"] = None if R == 1 or s_lo == 0 else s_hi / s_lo
    if f["rescue"] is None or f["self_consistency"] is None:
        f["verdict"] = "NA"
    else:
        f["verdict"] = ("fail", "borderline", "pass")[(hi < 2 * lo) + (s_hi < 2 * s_lo)]
    f["conservative"] = cons
    f["optimal"] = pooled if f["np"] > sum(cons) else cons
    return f


def _ratio(x):
    return "NA" if x is None else f"{x:.6f}"


def metrics_text(f):
    R = f["R"]
    rows, at = [("replicates", R)], 0
    for i in range(R):
        for j in range(i + 1, R):
            rows.append((f"Nt.t{i + 1}.t{j + 1}", f["nt_pair"][at]))
            at += 1
    rows += [("Nt", f["nt"] if R > 1 else "NA"), ("Np", f["np"])]
    rows += [(f"N_self.t{r + 1}", f["n_self"][r]) for r in range(R)]
    rows += [("rescue_ratio", _ratio(f["rescue"])), ("self_consistency_ratio", _ratio(f["self_consistency"])), ("verdict", f["verdict"]),
             ("conservative_peaks", sum(f["conservative"]) if R > 1 else "NA"), ("optimal_peaks", sum(f["optimal"]))]
    return "figure\tvalue\n" + "".join(f"{k}\t{v}\n" for k, v in rows)

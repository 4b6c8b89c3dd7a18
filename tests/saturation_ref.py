"""The subsample's draw and the saturation table's overlap figures once more, in numpy and by brute force: what
tests/test_saturation.py and tests/test_hip_saturation.py hold the library against (include/genrich_amd.h, gx_saturation)."""
import numpy as np

M64 = (1 << 64) - 1
FULL = 1 << 32          # the threshold that keeps every event


def draws(seed, sample, index):
    """The 32-bit draws of events `index` (an array) of kept sample `sample`, in uint64 arithmetic (numpy wraps it)."""
    i = np.asarray(index, dtype=np.uint64)
    key = np.uint64((int(seed) ^ (0x9E3779B97F4A7C15 * (int(sample) + 1))) & M64)
    with np.errstate(over="ignore"):
        x = key + i
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return (x >> np.uint64(32)).astype(np.uint64)


def draw(seed, sample, index):
    """One draw in Python's integers."""
    x = ((int(seed) ^ (0x9E3779B97F4A7C15 * (int(sample) + 1))) + int(index)) & M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x >> 32


def keep_mask(n, seed, sample, T):
    return draws(seed, sample, np.arange(n, dtype=np.uint64)) < np.uint64(T)


def subsample(ev, seed, k, T):
    """The events of `ev` (kept order) that sample k keeps at threshold T, in order."""
    return ev[keep_mask(len(ev), seed, k, T)]


def thresholds(n):
    return [(j << 32) // n for j in range(1, n + 1)]


def overlap(full, sub):
    """(full_recovered, sub_in_full, shared_bp) of two peak lists (records with chrom, start, end) by comparing every pair with
    the --counts predicate: s < pe and ps < e on one chromosome."""
    hit_f, hit_s, bp = set(), set(), 0
    for i, f in enumerate(full):
        for j, s in enumerate(sub):
            if f["chrom"] == s["chrom"] and int(s["start"]) < int(f["end"]) and int(f["start"]) < int(s["end"]):
                hit_f.add(i)
                hit_s.add(j)
                bp += min(int(f["end"]), int(s["end"])) - max(int(f["start"]), int(s["start"]))
    return len(hit_f), len(hit_s), bp

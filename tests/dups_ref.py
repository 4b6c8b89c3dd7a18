"""What gx_dups_first (include/genrich_amd.h) must return, in plain Python and in numpy, and the key sets on which
tests/test_dups_first.py (CPU: the two references against each other) and tests/test_hip_dups_first.py (GPU: the kernels
against them) run.  owner[i] = the index of the first record with record i's key, with bit 31 set when ANY record with that
key has multi != 0."""
import numpy as np

CONTESTED = 0x80000000
EDGE_WORDS = (0, 0xFFFFFFFF, 0x80000000)


def owner_dict(keys, multi):
    """A dict over key tuples: the first index per key, bit 31 when any record with the key is flagged."""
    keys = np.asarray(keys, dtype=np.uint32).reshape(-1, 4)
    first, flagged = {}, set()
    rows = [tuple(r) for r in keys.tolist()]
    for i, (k, m) in enumerate(zip(rows, np.asarray(multi).tolist())):
        first.setdefault(k, i)
        if m:
            flagged.add(k)
    return np.array([first[k] | (CONTESTED if k in flagged else 0) for k in rows], dtype=np.uint32)


def owner_np(keys, multi):
    """The same by np.unique over a 16-byte view of the keys (for the large cases)."""
    keys = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1, 4)
    n = len(keys)
    if not n:
        return np.zeros(0, dtype=np.uint32)
    _, first, inv = np.unique(keys.view(np.dtype((np.void, 16))).ravel(), return_index=True, return_inverse=True)
    inv = inv.ravel()
    flagged = np.zeros(len(first), dtype=bool)
    flagged[inv[np.asarray(multi).ravel() != 0]] = True
    return (first[inv].astype(np.uint32) | np.where(flagged[inv], CONTESTED, 0).astype(np.uint32)).astype(np.uint32)


# ---- the key sets: each returns (keys uint32 [n, 4], multi uint8 [n]) ---------------------------------------------------------

def distinct(n, seed=0):
    """n different keys that look like the host's: a tag, a chromosome, two coordinates."""
    rng = np.random.default_rng(1000 + seed)
    k = np.zeros((n, 4), dtype=np.uint32)
    k[:, 0] = 1 + np.arange(n) % 3
    k[:, 1] = rng.integers(0, 25, n)
    k[:, 2] = np.arange(n) * 7 + 11          # (different in every row)
    k[:, 3] = rng.integers(0, 1 << 28, n)
    return k, np.zeros(n, dtype=np.uint8)


def one_key(n, flag_last):
    k = np.tile(np.array([[3, 7, 123_456, 1]], dtype=np.uint32), (n, 1))
    m = np.zeros(n, dtype=np.uint8)
    if flag_last:
        m[-1] = 1
    return k, m


def heavy(n, seed=0):
    """n keys drawn from a pool of n / 4 and shuffled; multi on 3 % of the records."""
    rng = np.random.default_rng(2000 + seed)
    pool = distinct(n // 4, seed + 1)[0]
    k = pool[rng.integers(0, len(pool), n)]
    m = (rng.random(n) < 0.03).astype(np.uint8)
    return np.ascontiguousarray(k), m


def near_equal(seed=0):
    """Groups of keys that differ in exactly one of the four words (for each word), and groups that are the permutations of the same
    four words; the words include 0, 0xFFFFFFFF and 0x80000000; every key three times, shuffled; multi on one copy of a few keys."""
    import itertools
    rng = np.random.default_rng(3000 + seed)
    rows = []
    bases = [(5, 17, 1000, 2000), EDGE_WORDS + (1,), (0xFFFFFFFF,) * 4, (0, 0, 0, 0), (0x80000000, 0, 0x80000000, 0xFFFFFFFF)]
    for base in bases:
        rows.append(base)
        for w in range(4):
            for v in EDGE_WORDS + (base[w] ^ 1, base[w] ^ 0x80000000, (base[w] + 1) & 0xFFFFFFFF, (base[w] + (1 << 16)) & 0xFFFFFFFF):
                if v != base[w]:
                    rows.append(base[:w] + (v,) + base[w + 1:])
    for words in ((1, 2, 3, 4), EDGE_WORDS + (7,), (0, 0, 0xFFFFFFFF, 0xFFFFFFFF), (9, 9, 9, 0x80000000)):
        rows += list(itertools.permutations(words))
    uniq = sorted(set(rows))
    k = np.array(uniq * 3, dtype=np.uint32)
    m = np.zeros(len(k), dtype=np.uint8)
    m[rng.choice(len(k), len(uniq) // 5, replace=False)] = 1
    p = rng.permutation(len(k))
    return np.ascontiguousarray(k[p]), m[p]


def cluster(geometry, n_cluster=600, n_other=300, seed=0):
    """n_cluster distinct keys whose home slot is the LAST slot of the table that n = 2 * n_cluster + n_other records get, each
    twice, and n_other unrelated keys once: a probe chain n_cluster long that wraps to slot 0.  The homes come from
    `geometry(keys) -> (capacity, home)`, the library's own hash (gx_dups_geometry), and are asked again for the finished set.
    multi on one copy of a few cluster keys only.  Returns (keys, multi, is_cluster per record, capacity)."""
    rng = np.random.default_rng(4000 + seed)
    n = 2 * n_cluster + n_other
    cap = geometry(np.zeros((n, 4), dtype=np.uint32))[0]
    # candidates: a home slot is the hash's low bits, so the slot in the (larger) table of the candidates, masked, is the slot in
    # the table of `cap` slots -- checked below on the set itself
    n_cand = 5 * n_cluster * cap // 4
    cand = rng.integers(0, 1 << 32, (n_cand, 4), dtype=np.uint64).astype(np.uint32)
    cand[:, 0] = 1 + cand[:, 0] % 3
    big, home = geometry(cand)
    assert big >= cap
    cl = np.unique(cand[(home & (cap - 1)) == cap - 1], axis=0)
    assert len(cl) >= n_cluster, (len(cl), n_cand)
    cl = cl[rng.permutation(len(cl))[:n_cluster]]
    other = distinct(n_other, seed + 7)[0]
    other[:, 0] |= 0x100                      # (no cluster key has this bit: unrelated for sure)
    k = np.concatenate([cl, cl, other])
    is_cl = np.concatenate([np.ones(2 * n_cluster, dtype=bool), np.zeros(n_other, dtype=bool)])
    m = np.zeros(n, dtype=np.uint8)
    m[rng.choice(2 * n_cluster, 12, replace=False)] = 1
    p = rng.permutation(n)
    k, m, is_cl = np.ascontiguousarray(k[p]), m[p], is_cl[p]
    got_cap, got_home = geometry(k)
    assert got_cap == cap and (got_home[is_cl] == cap - 1).all()
    return k, m, is_cl, cap


def strided(n, stride, seed=0):
    """n records, stride < n <= 2 * stride: lane i of a grid of `stride` lanes takes record i and, on its second trip through the
    grid-stride loop, record i + stride.  A quarter of the first trip's records copy the key of an earlier one; of the second
    trip's (n - stride) records half copy a key of the first trip -- their first holder lies in the other trip --, a quarter copy
    an earlier record of the second trip and a quarter are new.  multi on 1 % of the records."""
    rng = np.random.default_rng(5000 + seed)
    idx = np.arange(n, dtype=np.uint64)
    k = np.zeros((n, 4), dtype=np.uint32)
    k[:, 0] = 3
    k[:, 1] = (idx & 0xFFFF).astype(np.uint32)
    k[:, 2] = (idx >> 16).astype(np.uint32)
    k[:, 3] = (idx * 2654435761 & 0xFFFFFFFF).astype(np.uint32)
    src = np.arange(n)
    dup = 1 + rng.choice(stride - 1, stride // 4, replace=False)
    src[dup] = rng.integers(0, dup)                                   # (any earlier record; chains of copies resolve below)
    tail = stride + rng.permutation(n - stride)
    a, b = tail[:len(tail) // 2], tail[len(tail) // 2: 3 * len(tail) // 4]
    src[a] = rng.integers(0, stride, len(a))
    b = b[b > stride]
    src[b] = rng.integers(stride, b)
    for _ in range(64):                                               # follow the copies to their roots
        nxt = src[src]
        if np.array_equal(nxt, src):
            break
        src = nxt
    k = np.ascontiguousarray(k[src])
    m = (rng.random(n) < 0.01).astype(np.uint8)
    return k, m

"""gx_sparse.h -- the sparse (key, sums...) lists of the per-sample figures (the complexity's multiplicities, the interval
lengths, the depth's deep list): folding a list that arrives in ascending order, and adding one list to another.

The header is host-only, so it runs in a program of its own (tests/sparse_main.cpp, its own main) compiled with
-fsanitize=address,undefined: any report makes the program fail.  What it prints is compared with a dict-based sum; every
figure is an integer, compared with ==."""
import os
import random
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = 2**64 - 1


def _cases():
    """(label, K, A, B): two lists of (key, v1..vK), each ascending in the key; keys may repeat."""
    def rows(keys, K, mul=1):
        return [(k,) + tuple(mul * (i + 1) + c for c in range(K)) for i, k in enumerate(keys)]

    out = []
    for K in (1, 2, 3):
        out += [
            (f"both empty, K={K}", K, [], []),
            (f"A empty, K={K}", K, [], rows([3, 5, 9], K)),
            (f"B empty, K={K}", K, rows([3, 5, 9], K), []),
            (f"disjoint, K={K}", K, rows([1, 2, 3], K), rows([10, 20, 30], K, 7)),
            (f"disjoint, B first, K={K}", K, rows([10, 20, 30], K), rows([1, 2, 3], K, 7)),
            (f"identical keys, K={K}", K, rows([4, 8, 15, 16], K), rows([4, 8, 15, 16], K, 100)),
            (f"interleaved, runs of equal keys in B, K={K}", K, rows([2, 4, 6, 8, 10], K), rows([1, 1, 1, 4, 4, 5, 10, 10, 11, 11], K, 50)),
            (f"runs in both, K={K}", K, rows([0, 0, 7, 7, 7], K), rows([7, 7, 9], K, 3)),
            (f"a single element in A, K={K}", K, rows([5], K), []),
            (f"a single element in B, K={K}", K, [], rows([5], K)),
            (f"a single element each, equal, K={K}", K, rows([5], K), rows([5], K, 9)),
            (f"a single element each, different, K={K}", K, rows([6], K), rows([5], K, 9)),
            (f"keys 0 and 2^64 - 1, K={K}", K, rows([0, 17, TOP], K), rows([0, TOP, TOP], K, 1000)),
            (f"key 2^64 - 1 only in B, K={K}", K, rows([0], K), rows([TOP], K)),
        ]
    rng = random.Random(20240611)
    for K in (1, 2, 3):
        for span in (40, 2000, TOP):   # many shared keys, few, none to speak of
            def draw(n):
                return sorted((rng.randrange(span + 1),) + tuple(rng.randrange(2**40) for _ in range(K)) for _ in range(n))
            out.append((f"random, keys up to {span}, K={K}", K, draw(rng.randrange(200, 400)), draw(rng.randrange(200, 400))))
    return out


def _sum(*lists):
    acc = {}
    for rows in lists:
        for r in rows:
            old = acc.get(r[0])
            acc[r[0]] = tuple(r[1:]) if old is None else tuple(x + y for x, y in zip(old, r[1:]))
    return [(k,) + acc[k] for k in sorted(acc)]


def test_sparse_standalone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sparse")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "sparse_main.cpp"), "-o", exe])
    cases = _cases()
    lines = []
    for label, K, A, B in cases:
        assert all(x[0] <= y[0] for rows in (A, B) for x, y in zip(rows, rows[1:])), label   # (the test's own inputs)
        lines.append(f"{K} {len(A)} {len(B)}")
        lines += [" ".join(str(v) for v in r) for r in A + B]
    spec = tmp_path / "spec.txt"
    spec.write_text("\n".join(lines) + "\n")
    res = subprocess.run([exe, str(spec)], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr)
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
    parts = res.stdout.split("--\n")
    assert len(parts) == 3 * len(cases) + 1 and parts[-1] == ""

    def parse(part, head):
        rows = part.splitlines()
        assert rows[0] == head, (rows[:1], head)
        return [tuple(int(v) for v in r.split()) for r in rows[1:]]

    for i, (label, K, A, B) in enumerate(cases):
        assert parse(parts[3 * i], "fold A") == _sum(A), label
        assert parse(parts[3 * i + 1], "fold B") == _sum(B), label
        assert parse(parts[3 * i + 2], "add") == _sum(A, B), label

#!/usr/bin/env python3
"""Two builds of genrich-amd on the same random command lines: exit status, stdout, stderr and the files left behind must agree.

    tools/fuzz_host_argv.py OLD_BIN NEW_BIN SEED0 SEED1 [--replay]

One argv per seed in SEED0 .. SEED1 - 1, made of the long options' names (read from the table in genrich_amd/host/host_options.h),
the short options, -h, -V, the --help-* options, abbreviated long options, --opt=value and stray arguments; values come from a short
list (valid, out of range, malformed, empty).  --replay runs every argv of tests/test_host_refusals.py as well.  Each binary runs in
a directory of its own that holds one small SAM file and one BED.  For a machine without a GPU: a run that gets as far as making a
device context fails there, with the same message from both builds.  Not a test; prints the differences and exits 1 if there are any."""
import os
import random
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = open(os.path.join(ROOT, "genrich_amd", "host", "host_options.h")).read()
LONG = re.findall(r'^    \{"([a-z0-9-]+)", (no|required)_argument', TABLE, re.M)      # (name, takes an argument)
SHORT = "ht:c:o:f:k:b:zyw:xjd:De:E:m:s:p:q:a:l:g:rR:XPSL:vV"
SHORT = [(m.group(1), bool(m.group(2))) for m in re.finditer(r"([A-Za-z])(:?)", SHORT)]
VALUES = ["t.sam", "a.bed", "out.x", "pre", "", "0", "1", "2", "50", "100", "101", "4096", "4097", "-1", "+5", "5x", "5 ", " 5", "x", "0.5", "1e-4",
          "nan", "inf", "1e400", "99999999999999999999", "18446744073709551615", "0,0", "0-1", "0,1", "100,200", "200,100", "-50,400", "tss",
          "center", "null", "t.sam,t.sam", "-", "-x"]
SAM = ("@HD\tVN:1.0\tSO:queryname\n@SQ\tSN:chr1\tLN:10000\n"
       + "".join(f"r{i}\t99\tchr1\t{100 + 7 * i}\t30\t50M\t=\t{250 + 7 * i}\t200\t*\t*\nr{i}\t147\tchr1\t{250 + 7 * i}\t30\t50M\t=\t{100 + 7 * i}\t-200\t*\t*\n"
                 for i in range(40)))
BED = "chr1\t100\t600\tsite\t0\t+\nchr2\t5\t50\n"


def argv_of(seed):
    rng = random.Random(seed)
    argv = []
    if rng.random() < 0.8:      # most command lines name their files: the others end at "Need input/output files"
        argv += rng.choice([["-t", "t.sam", "-o", "o.np"], ["--events-only", "-t", "t.sam"], ["-P", "-f", "l.log", "-o", "o.np"], ["-X", "-t", "t.sam"],
                            ["--events-only", "-t", "t.sam", "-b", "o.bed"]])
    for _ in range(rng.choice([0, 1, 1, 2, 2, 3, 4, 6])):
        if rng.random() < 0.75:
            name, arg = rng.choice(LONG)
            arg = arg == "required"
            if rng.random() < 0.15:
                name = name[:rng.randint(2, len(name))]     # an abbreviation: unique, ambiguous or the whole name
            if not arg:
                argv.append("--" + name)
            elif rng.random() < 0.3 and name != "threads":
                argv.append(f"--{name}={rng.choice(VALUES)}")
            elif name.startswith("threads"[:len(name)]):
                argv += ["--" + name, rng.choice(["1", "2", "4", "x", ""])]      # (no thousands of threads)
            else:
                argv += ["--" + name, rng.choice(VALUES)]
        else:
            name, arg = rng.choice(SHORT)
            argv += ["-" + name] + ([rng.choice(VALUES)] if arg else [])
        if rng.random() < 0.04:
            argv.append(rng.choice(["stray", "--", "--no-such-option", "-Z"]))
    if rng.random() < 0.1:
        rng.shuffle(argv)
    return argv


def outcome(binary, argv):
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.sam"), "w").write(SAM)
        open(os.path.join(d, "a.bed"), "w").write(BED)
        env = {k: v for k, v in os.environ.items() if not k.startswith("GENRICH_")}
        res = subprocess.run(["genrich-amd"] + argv, executable=binary, cwd=d,       # (getopt's own messages begin with argv[0])
                             capture_output=True, env=env, stdin=subprocess.DEVNULL, timeout=120)
        files = {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}
    return res.returncode, res.stdout, res.stderr, files


def main():
    replay = "--replay" in sys.argv
    old, new, seed0, seed1 = [a for a in sys.argv[1:] if a != "--replay"]
    old, new = os.path.abspath(old), os.path.abspath(new)
    cases = [(f"seed {s}", argv_of(s)) for s in range(int(seed0), int(seed1))]
    if replay:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import test_host_refusals
        cases += [(name, argv) for name, (argv, _) in test_host_refusals.CASES.items()]
    different, status = 0, {}
    for name, argv in cases:
        a, b = outcome(old, argv), outcome(new, argv)
        status[a[0]] = status.get(a[0], 0) + 1
        if a != b:
            different += 1
            print(f"DIFFERENT, {name}: {argv!r}\n  old: {a[:3]!r} {sorted(a[3])}\n  new: {b[:3]!r} {sorted(b[3])}")
    print(f"{len(cases)} command lines, {different} different; exit statuses of the old build: {dict(sorted(status.items()))}")
    return 1 if different else 0


if __name__ == "__main__":
    sys.exit(main())

"""A/B timing on the GPU box: python tools/ab.py [--rounds N] [--args "<bench args>"] [--key roofline.kernel_ms] name=ENV1=V1,ENV2=V2 ...
Each variant is a set of environment variables (e.g. SGW_LIB=..., SGW_NO_FUSED=1); variants are run
interleaved for N rounds; prints min / median / max of each (the key of bench.py's line, in us), then for every variant against
the FIRST one whether all of its runs lie below all of the first's, and -- where two variants have the same environment (an A/A
pair) -- the spread between their medians: the noise the differences above have to be read against."""
import json
import os
import subprocess
import sys

rounds, bargs, variants, key = 4, "", [], "roofline.kernel_ms"
it = iter(sys.argv[1:])
for a in it:
    if a == "--rounds":
        rounds = int(next(it))
    elif a == "--args":
        bargs = next(it)
    elif a == "--key":
        key = next(it)
    else:
        name, _, envs = a.partition("=")
        variants.append((name, dict(e.split("=", 1) for e in envs.split(",") if e)))
base = ["--no-cpu-baseline", "--no-series", "--prewarm-steps", "300", "--steps", "300"]
if not key.startswith("roofline.kernel_ms"):
    base = ["--no-cpu-baseline", "--no-series", "--full", "--side-steps", "20", "--steps", "300"]   # (the policy-turn leg runs with the side configs)
res = {n: [] for n, _ in variants}
for r in range(rounds):
    for name, env in variants:
        out = subprocess.run([sys.executable, "bench.py"] + base + bargs.split(),
                             env={**os.environ, **env}, capture_output=True, text=True).stdout.strip().splitlines()[-1]
        v = json.loads(out)
        for k in key.split("."):
            v = v[k]
        res[name].append(v * 1000)
        print(f"round {r} {name}: {v * 1000:.2f}", flush=True)


def med(v):
    return sorted(v)[len(v) // 2]


for name, v in res.items():
    v2 = sorted(v)
    print(f"{name:12s} min {v2[0]:7.1f}  med {med(v):7.1f}  max {v2[-1]:7.1f} us   {['%.1f' % x for x in v]}")
first = variants[0][0]
for name, _ in variants[1:]:
    below, above = max(res[name]) < min(res[first]), min(res[name]) > max(res[first])
    print(f"{name} vs {first}: median {100 * (med(res[name]) / med(res[first]) - 1):+.2f} %; every run below every run of {first}: {'yes' if below else 'no'}"
          + ("; EVERY RUN ABOVE" if above else ""))
for i, (n1, e1) in enumerate(variants):
    for n2, e2 in variants[i + 1:]:
        if e1 == e2:
            print(f"A/A {n1} / {n2}: medians {med(res[n1]):.1f} / {med(res[n2]):.1f} us = {100 * abs(med(res[n1]) / med(res[n2]) - 1):.2f} % spread")

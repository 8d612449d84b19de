"""Two builds of libflowstate.so on tools/rkld_ab.py's graphed training step at ALPHA = 0.5 (batch 256,
the A2 flow), alternating processes.

    tools/rkld_lib_ab.py LIB_A LIB_B [--shapes a2] [--rounds 4] [--out ab.json]

Round r runs rkld_ab.py once with FLOWSTATE_LIB=LIB_A and once with LIB_B (a process each, in this
order: A B A B ...).  Per case (shape / fused or per-op sampling backward) and build: the ms per step
of every round, their median and their spread (max - min).  B counts as no slower than A when its
median exceeds A's by no more than the two spreads together (exit status 2 otherwise).  One JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def one(lib, shapes, steps, inner):
    env = dict(os.environ, FLOWSTATE_LIB=os.path.abspath(lib))
    out = subprocess.run([sys.executable, os.path.join(HERE, "rkld_ab.py"), "--shapes", shapes, "--rounds", str(inner),
                          "--steps", str(steps)], env=env, check=True, timeout=600, stdout=subprocess.PIPE,
                         text=True).stdout
    res = json.loads([l for l in out.splitlines() if l.startswith("{")][0])["cases"]
    return {c: res[c]["ms_per_step"] for c in res}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("lib_a")
    ap.add_argument("lib_b")
    ap.add_argument("--shapes", default="a2")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--inner-rounds", type=int, default=3, help="--rounds of each rkld_ab.py process")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out")
    a = ap.parse_args()
    libs = {"a": a.lib_a, "b": a.lib_b}
    ms = {k: {} for k in libs}
    for r in range(a.rounds):
        for k, lib in libs.items():
            got = one(lib, a.shapes, a.steps, a.inner_rounds)
            for c, v in got.items():
                ms[k].setdefault(c, []).append(round(v, 4))
            print("round %d %s %s" % (r, k, json.dumps(got)), file=sys.stderr, flush=True)
    res = {"metric": "ms per graphed training step at ALPHA = 0.5, batch 256 (tools/rkld_ab.py), one process per "
                     "entry, alternating", "lib_a": a.lib_a, "lib_b": a.lib_b, "rounds": a.rounds, "cases": {}}
    for c in ms["a"]:
        st = {k: {"ms": ms[k][c], "median": statistics.median(ms[k][c]), "spread": max(ms[k][c]) - min(ms[k][c])}
              for k in libs}
        allowed = st["a"]["spread"] + st["b"]["spread"]
        res["cases"][c] = {**st, "b_minus_a": st["b"]["median"] - st["a"]["median"], "allowed": allowed,
                           "b_no_slower": st["b"]["median"] - st["a"]["median"] <= allowed}
    res["b_no_slower"] = all(v["b_no_slower"] for v in res["cases"].values())
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["b_no_slower"] else 2


if __name__ == "__main__":
    sys.exit(main())

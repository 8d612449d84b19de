#!/usr/bin/env python3
"""Compare the kernels of two device-assembly files (hipcc --cuda-device-only -S) one by one.

    tools/kernel_asm_diff.py parent.s new.s [--rename REGEX=REPL ...] [--must-match REGEX ...]

Kernels are paired by symbol; --rename rewrites the first file's symbols first (re.sub), for a
kernel whose name or signature changed.  Of each kernel the instruction stream (comments
stripped, the function number taken out of local labels) and the .amdhsa_* figures are compared,
and one verdict is printed:

    identical                       same stream, same figures
    same opcodes, order differs     the same multiset of opcodes in another order (or with other
                                    operands); figures that differ are listed
    different                       with line counts, VGPRs, scratch, the opcode counts and the
                                    figures that differ

Exit status 1 if a kernel whose (renamed) symbol matches a --must-match pattern is not identical
or has no partner, else 0.  The tool knows no instruction: it only diffs.
"""
import argparse
import collections
import re
import sys

_LABEL_NO = re.compile(r"\.L(BB|func_(?:begin|end)|tmp)\d+")


def parse(text):
    """{symbol: (instruction lines, {amdhsa figure: value})} of the kernels in an assembly text."""
    streams, figures = {}, {}
    body = desc = None
    for raw in text.splitlines():
        line = raw.split(";", 1)[0].strip()
        if not line:
            continue
        if desc is not None:  # inside .amdhsa_kernel ... .end_amdhsa_kernel
            if line == ".end_amdhsa_kernel":
                desc = None
            else:
                key, _, value = line.partition(" ")
                figures[desc][key] = value.strip()
        elif line.startswith(".amdhsa_kernel "):
            desc = line.split()[1]
            figures[desc] = {}
        elif body is not None:
            if line.startswith(".Lfunc_end"):
                body = None
            elif line.endswith(":") or not line.startswith("."):  # a label or an instruction
                streams[body].append(_LABEL_NO.sub(r".L\1", " ".join(line.split())))
        elif re.fullmatch(r"[A-Za-z_][\w$.]*:", line):
            body = line[:-1]
            streams[body] = []
    return {s: (streams.get(s, []), f) for s, f in figures.items()}


def opcodes(stream):
    return collections.Counter(l.split()[0] for l in stream if not l.endswith(":"))


def compare(a, b):
    """(verdict, detail) for two parsed kernels."""
    (sa, fa), (sb, fb) = a, b
    figs = ["%s %s -> %s" % (k[len(".amdhsa_"):], fa.get(k, "-"), fb.get(k, "-"))
            for k in sorted(set(fa) | set(fb)) if fa.get(k) != fb.get(k)]
    if sa == sb and not figs:
        return "identical", "%d lines" % len(sa)
    oa, ob = opcodes(sa), opcodes(sb)
    if sa != sb and oa == ob:
        moved = sum(x != y for x, y in zip(sa, sb))  # same multiset of opcodes: same number of lines
        return "same opcodes, order differs", "; ".join(["%d of %d lines differ in place" % (moved, len(sa))] + figs)
    detail = ["stream identical" if sa == sb else "lines %d -> %d" % (len(sa), len(sb))]
    for name, key in (("VGPR", ".amdhsa_next_free_vgpr"), ("scratch", ".amdhsa_private_segment_fixed_size")):
        detail.append("%s %s -> %s" % (name, fa.get(key, "-"), fb.get(key, "-")))
    ops = ["%s %+d" % (o, ob[o] - oa[o]) for o in sorted(set(oa) | set(ob)) if oa[o] != ob[o]]
    if ops:
        detail.append("opcodes: " + ", ".join(ops))
    return "different", "; ".join(detail + figs)


def diff(text_a, text_b, renames=(), must_match=()):
    """([(symbol, verdict, detail)], failed symbols)"""
    ka = {}
    for sym, k in parse(text_a).items():
        for pat, repl in renames:
            sym = re.sub(pat, repl, sym)
        ka[sym] = k
    kb = parse(text_b)
    rows, failed = [], []
    for sym in sorted(set(ka) | set(kb)):
        if sym in ka and sym in kb:
            verdict, detail = compare(ka[sym], kb[sym])
        else:
            verdict, detail = "only in the %s file" % ("first" if sym in ka else "second"), ""
        rows.append((sym, verdict, detail))
        if verdict != "identical" and any(re.search(p, sym) for p in must_match):
            failed.append(sym)
    return rows, failed


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("first")
    ap.add_argument("second")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL",
                    help="rewrite the first file's symbols before pairing")
    ap.add_argument("--must-match", action="append", default=[], metavar="REGEX",
                    help="kernels that have to be identical")
    args = ap.parse_args(argv)
    renames = [tuple(r.split("=", 1)) for r in args.rename]
    with open(args.first) as fa, open(args.second) as fb:
        rows, failed = diff(fa.read(), fb.read(), renames, args.must_match)
    for sym, verdict, detail in rows:
        print("%s: %s%s" % (sym, verdict, " (%s)" % detail if detail else ""))
    count = collections.Counter(v for _, v, _ in rows)
    print("# %d kernels: %s" % (len(rows), ", ".join("%d %s" % (n, v) for v, n in sorted(count.items()))))
    for sym in failed:
        print("# must match, does not: %s" % sym)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())

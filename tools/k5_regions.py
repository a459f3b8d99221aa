"""Scheduling regions of K5's compiled pair loop (gfx950).

For one instantiation of `k5_fused` (default: <64, false, false, false>, the
benchmark's) in a built libtritd.so or object file, finds the walk's main loop
— the innermost loop with the most MFMAs: two t-tiles per trip —
and reports every conditional branch in it and what lies between them: per
straight-line region the instruction counts by class and its memory / MFMA
events in issue order, run-length coded:

    M  v_mfma_*            d  ds_read* / ds_bpermute    D  ds_write*
    l  buffer/global load  S  buffer/global store       b  s_barrier

so that one can read off whether the compact-E decode's LDS round trips sit
between the MFMAs of the L chain, and what separates the Y_L store from the
slot store.  A region ends at a conditional branch, or at a
label some branch of the loop jumps to; `s_and_saveexec` is listed with the
branches' count as `saveexec` (it opens a lane-masked stretch, usually closed
by a branch).

    python tools/k5_regions.py [--json] [--kernel SUBSTR] [lib.so | object.o]

The last line, `cbranch N`, is the figure tests/test_k5_regions.py holds the
built library to (profiles/k5_step_regions/regions_branch.txt).
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import scan_store_war as sw  # noqa: E402

KERNEL = "k5_fusedILi64ELb0ELb0ELb0EE"
CLASSES = ("mfma", "valu_f64", "valu", "salu", "waitcnt", "lds", "vmem")


def classify(mn):
    if mn.startswith("v_mfma"):
        return "mfma"
    if mn == "s_waitcnt":
        return "waitcnt"
    if mn.startswith("ds_"):
        return "lds"
    if mn.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    if mn.startswith("v_"):
        return "valu_f64" if re.search(r"_f64|_u64|_i64|_b64", mn) else "valu"
    if mn.startswith("s_"):
        return "salu"
    return "other"


def event(mn):
    if mn.startswith("v_mfma"):
        return "M"
    if mn.startswith(("ds_write", "ds_store")):
        return "D"
    if mn.startswith("ds_"):
        return "d"
    if mn.startswith(("buffer_store", "global_store", "flat_store")):
        return "S"
    if mn.startswith(("buffer_load", "global_load", "flat_load")):
        return "l"
    if mn == "s_barrier":
        return "b"
    return ""


def rle(s):
    out = []
    for m in re.finditer(r"(.)\1*", s):
        n = len(m.group(0))
        out.append(m.group(1) + (str(n) if n > 1 else ""))
    return " ".join(out)


def find_kernel(path, sub=KERNEL):
    for blob in sw.code_objects(path):
        for f, ins in sw.parse(sw.disassemble(blob)).items():
            if sub in f and not f.endswith(".kd"):
                return f, ins
    raise SystemExit("no kernel matching %r in %s" % (sub, path))


def is_cbranch(mn):
    return mn.startswith("s_cbranch")


def pair_loop(ins):
    """(first, last) instruction indices of the innermost loop (a backward
    branch's span with no other backward branch inside) with the most MFMAs."""
    index = {a: n for n, (a, _, _) in enumerate(ins)}
    spans = []
    for n, (addr, mn, ops) in enumerate(ins):
        if not sw._BR.match(mn):
            continue
        tgt = sw.branch_target(mn, ops, addr)
        if tgt is not None and tgt in index and index[tgt] <= n:
            spans.append((index[tgt], n))
    best = None
    for k, n in spans:
        if any((k2, n2) != (k, n) and k <= k2 and n2 <= n for k2, n2 in spans):
            continue
        mf = sum(1 for _, m, _ in ins[k:n + 1] if m.startswith("v_mfma"))
        if best is None or mf > best[0]:
            best = (mf, k, n)
    if best is None:
        raise SystemExit("no loop found")
    return best[1], best[2]


def regions(ins, first, last):
    """The loop's straight-line regions: [dict(start, end_by, counts, events)]."""
    index = {a: n for n, (a, _, _) in enumerate(ins)}
    labels = set()
    for n in range(first, last + 1):
        addr, mn, ops = ins[n]
        if sw._BR.match(mn):
            tgt = sw.branch_target(mn, ops, addr)
            if tgt in index and first <= index[tgt] <= last:
                labels.add(index[tgt])
    out, cur = [], None

    def close(end_by):
        nonlocal cur
        if cur is not None:
            cur["end_by"] = end_by
            cur["events"] = rle(cur["events"])
            out.append(cur)
        cur = None

    for n in range(first, last + 1):
        addr, mn, ops = ins[n]
        if n in labels and cur is not None and cur["n"]:
            close("label")
        if cur is None:
            cur = dict(start="0x%x" % addr, n=0, counts={c: 0 for c in CLASSES}, events="", saveexec=0)
        cur["n"] += 1
        c = classify(mn)
        if c in cur["counts"]:
            cur["counts"][c] += 1
        cur["events"] += event(mn)
        if "saveexec" in mn:
            cur["saveexec"] += 1
        if is_cbranch(mn) or mn == "s_branch":
            close(mn)
    close("end")
    return out


def report(path, sub=KERNEL):
    name, ins = find_kernel(path, sub)
    first, last = pair_loop(ins)
    regs = regions(ins, first, last)
    total = {c: sum(r["counts"][c] for r in regs) for c in CLASSES}
    return dict(kernel=name, loop_start="0x%x" % ins[first][0], loop_end="0x%x" % ins[last][0],
                instructions=last - first + 1, totals=total,
                cbranch=sum(1 for r in regs if r["end_by"].startswith("s_cbranch")),
                saveexec=sum(r["saveexec"] for r in regs), regions=regs)


def main():
    args = sys.argv[1:]
    as_json = "--json" in args
    args = [a for a in args if a != "--json"]
    sub = KERNEL
    if "--kernel" in args:
        k = args.index("--kernel")
        sub = args[k + 1]
        del args[k:k + 2]
    path = args[0] if args else os.path.join(sw.CSRC, "..", "tritd", "libtritd.so")
    rep = report(path, sub)
    if as_json:
        print(json.dumps(rep, indent=1))
        return 0
    print("%s\npair loop %s..%s: %d instructions" % (rep["kernel"], rep["loop_start"], rep["loop_end"],
                                                     rep["instructions"]))
    print("totals  " + "  ".join("%s %d" % (c, rep["totals"][c]) for c in CLASSES))
    for n, r in enumerate(rep["regions"]):
        print("region %2d at %s: %3d instructions, ends by %s%s" %
              (n, r["start"], r["n"], r["end_by"], "  (saveexec %d)" % r["saveexec"] if r["saveexec"] else ""))
        print("    " + "  ".join("%s %d" % (c, r["counts"][c]) for c in CLASSES if r["counts"][c]))
        if r["events"]:
            print("    " + r["events"])
    print("saveexec %d" % rep["saveexec"])
    print("cbranch %d" % rep["cbranch"])
    return 0


if __name__ == "__main__":
    sys.exit(main())

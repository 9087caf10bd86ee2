"""Dynamic instruction table of lqr_qtol_kernel<3,12,7,40> for the bench shape (4096 IK problems, n = 40, 5 x 12 rows, ranks 12, 12, 12, 4, 0),
from assembly alone: no GPU needed.

The kernel is unrolled straight-line code, so its dynamic instruction count is the static count of each part times the number of times the
bench shape runs that part.  A build with -DLEXLS_QTOL_MARKS puts a comment "; qtol-region <name> [i [j]]" at the head of every phase and
of every unrolled step (lqr_qtol_impl.h); this script cuts the assembly at those comments (a part = the text from its mark to the next one),
counts instructions per class and weighs every part with its trip count.  The marks emit no instruction; that they change no vector or
memory instruction either is checked against the product assembly the Makefile leaves behind, when that file is given as well.

  make -C lexls_amd/csrc lqr_qtol_3x12s7.marks.s
  python scripts/qtol_insn_table.py lexls_amd/csrc/lqr_qtol_3x12s7.marks.s [lexls_amd/csrc/lqr_qtol_3x12s7.s] [--md title] > profiles/qtol_insn_table_<when>.md
"""
import collections
import re
import sys

CLASSES = ["fma/mul/add f64", "fmac dpp", "v_cndmask", "dpp move", "v_accvgpr", "other VALU", "LDS", "global", "SALU", "wait/nop"]
VALU = CLASSES[:6]


def classify(m):
    if m.startswith("v_fmac_f64_dpp"):
        return "fmac dpp"
    if re.match(r"v_(fma|fmac|mul|add|max|min)_f64", m) and not m.endswith("_dpp"):
        return "fma/mul/add f64"
    if m.startswith("v_cndmask"):
        return "v_cndmask"
    if m.startswith("v_mov_b64_dpp") or m.startswith("v_mov_b32_dpp"):
        return "dpp move"
    if m.startswith("v_accvgpr"):
        return "v_accvgpr"
    if m.startswith("v_"):
        return "other VALU"  # integer, compare, v_perm, readlane, v_max_f64_dpp of the butterflies, rsq / rcp, plain moves
    if m.startswith("ds_"):
        return "LDS"
    if m.startswith(("global_", "flat_", "buffer_")):
        return "global"
    if m in ("s_waitcnt", "s_nop"):
        return "wait/nop"
    if m.startswith("s_"):
        return "SALU"
    return None


# the instantiation and the shape the table is for: lqr_qtol_kernel<NS, MD, SIG, N> on ranks RANKS (bench.py's batch)
NS, MD, SIG, N = 3, 12, 7, 40
RANKS = [12, 12, 12, 4, 0]
FC = [sum(RANKS[:k]) for k in range(len(RANKS))]          # first column of every level: 0, 12, 24, 36, 40
WORKED = [k for k in range(len(RANKS)) if FC[k] < N]      # levels that start (x only: once the columns are exhausted nothing is done)
S0 = [min((FC[k] + SIG) // 16, NS - 1) for k in WORKED]   # first live slot = the factor_level instantiation of the level
# levels that retire their low slot behind the first pivot step (the body's RETIRE): two live slots, the level's first column in lane 15 of the
# lower one.  They run the "hh-ret-*" parts (the retiring form of factor_level<S0>) instead of "hh-*"
RET = [k != 0 and S0[WORKED.index(k)] == NS - 2 and (FC[k] + SIG) % 16 == 15 for k in WORKED]
ACC = [N - (FC[k] + RANKS[k]) if RANKS[k] else 0 for k in range(len(RANKS))]  # solved positions behind a level's pivots (back-substitution)


def trips(name, idx):
    """how often the shape runs a part.  Level 0 is a peeled section in front of the level loop: its parts are marked "level0-<name>" and run
    once; the same name without the prefix is the part of the loop's body, which serves the levels behind level 0"""
    if name in ("prologue", "solve-top", "output"):
        return 1
    if name in ("solve-level",):
        return len(RANKS)
    if name == "solve-tail":
        return sum(1 for r in RANKS if r)
    if name == "solve-trip":
        return sum(-(-a // 16) for a in ACC)
    l0 = name.startswith(L0_PREFIX)
    if l0:
        name = name[len(L0_PREFIX):]
    levels = [k for k in WORKED if (k == 0) == l0]  # the levels that run this copy of the part
    if name == "level-top":
        return 1 if l0 else len(RANKS) - 1  # (a level that does not start leaves at once)
    if name in ("level-start", "level-stage", "level-post", "hh-select", "level-end", "level-end-maps"):
        return len(levels)  # (level-start, level-stage, hh-select: the loop only — level 0 is loaded in the position layout directly and has one instantiation)
    if name == "level-end-store":  # slot s holds a live column (position 16 s + l - SIG >= Fc) in some lane: otherwise the pass is branched over
        return sum(1 for k in levels if 16 * idx[0] + 15 - SIG >= FC[k])
    if name == "elim":
        return sum(1 for k in levels if idx[0] < FC[k])
    ret = name.startswith("hh-ret")  # the retiring form's parts; "hh-retire": the move behind its step 0 (run with that step)
    if ret:
        name = {"hh-ret-pro": "hh-pro", "hh-ret-end": "hh-end", "hh-ret-step": "hh-step", "hh-retire": "hh-step"}[name]
        if len(idx) == 1 and name == "hh-step":
            idx = (idx[0], 0)
    levels = [k for k in levels if RET[WORKED.index(k)] == ret] if name.startswith("hh-") else levels
    if name in ("hh-pro", "hh-end"):
        return sum(1 for k in levels if S0[WORKED.index(k)] == idx[0])
    if name == "hh-step":  # a level leaves at the first test (every fourth step) behind its last pivot
        s0, j = idx
        return sum(1 for k in levels if S0[WORKED.index(k)] == s0 and j < min(MD, -(-min(RANKS[k] + (FC[k] + RANKS[k] < N), MD) // 4) * 4))
    raise SystemExit(f"unknown region {name}")


L0_PREFIX = "level0-"


def group(name, idx):
    if name.startswith(L0_PREFIX):
        return "level 0 (peeled): " + group(name[len(L0_PREFIX):], idx)
    if name == "elim":
        sc = (idx[0] + SIG) // 16
        return f"elimination, {NS - sc} slot step"
    if name.startswith("hh-ret"):
        return f"Householder, factor_level<{idx[0]}> retiring slot {idx[0]} behind step 0"
    if name.startswith("hh-"):
        return f"Householder, factor_level<{idx[0]}>" if name != "hh-select" else "Householder, choice of the instantiation"
    if name.startswith("level-st"):
        return "level start"
    if name in ("level-top", "level-post"):
        return "level head (bookkeeping, prefetch test, first U')"
    if name.startswith("level-end"):
        return "level end"
    if name.startswith("solve"):
        return "back-substitution"
    return {"prologue": "prologue (first level's loads, LDS set-up)", "output": "results"}[name]


def parse(path, want_marks):
    """[(name, idx, Counter of classes)] of the first kernel of the file"""
    parts = [("prologue", (), collections.Counter())]
    inside = False
    for line in open(path):
        t = line.strip()
        if inside and t.startswith(".Lfunc_end"):
            break
        if re.match(r"_Z\w*lqr_qtol_kernel\w*:", t):
            inside = True
            continue
        if not inside:
            continue
        m = re.match(r"; qtol-region (\S+)((?: \d+)*)$", t)
        if m:
            parts.append((m.group(1), tuple(int(v) for v in m.group(2).split()), collections.Counter()))
            continue
        if not t or t[0] in ";." or t.endswith(":"):
            continue
        c = classify(t.split()[0])
        if c:
            parts[-1][2][c] += 1
    if want_marks and len(parts) < 10:
        raise SystemExit(f"{path}: no region marks — compile with -DLEXLS_QTOL_MARKS")
    return parts


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("marked", help="assembly of a -DLEXLS_QTOL_MARKS build (make -C lexls_amd/csrc lqr_qtol_3x12s7.marks.s)")
    ap.add_argument("product", nargs="?", help="the product assembly the Makefile leaves behind, to check the marked one against")
    ap.add_argument("--md", metavar="TITLE", help="title of the table")
    a = ap.parse_args()
    args = [a.marked] + ([a.product] if a.product else [])
    title = a.md or a.marked
    parts = parse(args[0], True)
    static = collections.Counter()
    for _, _, c in parts:
        static.update(c)
    if len(args) > 1:
        prod = collections.Counter()
        for _, _, c in parse(args[1], False):
            prod.update(c)
        same = ("LDS", "global") + tuple(VALU)  # (the marks end basic blocks: a few scalar branches and waits differ, no vector or memory instruction may)
        if any(prod[k] != static[k] for k in same):
            raise SystemExit(f"the marked assembly is not the product's: {dict(static)} against {dict(prod)}")
    rows = collections.OrderedDict()
    steps = collections.Counter()
    for name, idx, c in parts:
        g = group(name, idx)
        n = trips(name, idx)
        r = rows.setdefault(g, collections.Counter())
        for k, v in c.items():
            r[k] += n * v
        if name in ("elim", "hh-step", "hh-ret-step", L0_PREFIX + "hh-step"):
            steps[g] += n
    total = collections.Counter()
    for r in rows.values():
        total.update(r)
    print(f"# lqr_qtol_kernel<3,12,7,40>: instructions per wavefront on the bench shape — {title}\n")
    print("Static count of each part of the assembly times the part's trip count for ranks 12, 12, 12, 4, 0 (`scripts/qtol_insn_table.py`).")
    print("A part is counted whole: what the shape branches over inside one is counted as run (see the note below the table).\n")
    print("| part | steps | " + " | ".join(CLASSES) + " | VALU |")
    print("|---|---:|" + "---:|" * (len(CLASSES) + 1))
    for g in sorted(rows):
        r = rows[g]
        print(f"| {g} | {steps[g] or ''} | " + " | ".join(str(r[k]) for k in CLASSES) + f" | {sum(r[k] for k in VALU)} |")
    print("| **total** | | " + " | ".join(str(total[k]) for k in CLASSES) + f" | **{sum(total[k] for k in VALU)}** |")
    print(f"\nStatic histogram of the kernel: " + ", ".join(f"{k} {static[k]}" for k in CLASSES) + ".")
    hh_last = sum(c["global"] for name, idx, c in parts if name in ("hh-step", "hh-end") and idx[0] == S0[-1] and trips(name, idx))
    print(f"\nNote. The parent's measured count is 11,595 vector instructions per wavefront (SQ_INSTS_VALU / SQ_WAVES, profiles/r04_summary.md); a table that")
    print("comes out a few percent above it counts code the shape branches over inside a part. Known of that kind: the per-lane `if (mv)` store pass")
    print("of a level-end slot is weighed by the levels in which the slot holds a live column (its marks are per slot), but the address and select")
    print("instructions the compiler hoists in front of the branch are counted for every level; the requests for the next level's rows inside the")
    print(f"last level's pivot steps ({hh_last} global loads with their address arithmetic) are skipped there (`prefetch` is false); the fifth level leaves")
    print("`level-top` after a ballot. Instructions also move between neighbouring parts with the scheduler (the first U' fetch between level head")
    print("and the first elimination step): compare totals and the parts that changed, not single cells of unchanged parts.")
    if len(args) > 1:
        print("The marked build and the product build have the same vector, LDS and global-memory instructions.")


if __name__ == "__main__":
    main()

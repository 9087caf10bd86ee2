"""The large path's host-side plan (lexls_amd/csrc/lqr_large_plan.h) on its own, on the host, through tests/large_plan_check.cpp: the work
space of the step-per-pivot form is laid out ONCE (fast_workspace_layout) and the launcher, the clearing in front of a one-launch level and
large_fast_workspace_bytes all read that layout — here it is checked against what the kernels need of each piece, and its total against the
sum formula of the commit before the layout existed (PARENT_TOTAL: that formula evaluated for these shapes, `+ 256 ... + 64` of slack
included; the handle reuses a work space whenever the total fits, so the total may shrink but never grow).  No GPU needed.

Shapes: the seven cases of tests/large_cases.py as batches and problem by problem; largest level dimensions 0 and 1; n = 1, 1019, 1020, 1021
and 1024 around the 256 workgroups the one-launch form may have (G = 1, 255, 256, 256, 257)."""
import large_cases as L
import large_plan as LP


def shapes():
    """(batch, n, cap, rows_max, level_max) per shape"""
    out = []
    for c in L.CASES.values():
        dims = [d for d, _ in c["problems"]]
        for group in [dims] + [[d] for d in dims]:
            out.append((len(group), c["n"], sum(c["dims"]), max(sum(d) for d in group), [max(col) for col in zip(*group)]))
    for maxdim in (0, 1):
        for batch in (1, 3):
            out.append((batch, 60, 80, 2 * maxdim, [maxdim, maxdim]))
    for n in (1, 1019, 1020, 1021, 1024):
        for batch in (1, 2):
            out.append((batch, n, 80, 80, [40, 40]))
    return out


# (batch, n, cap, maxdim) -> large_fast_workspace_bytes of the parent commit
PARENT_TOTAL = {
    (3, 60, 1100, 1030): 27615224,
    (1, 60, 1100, 1030): 9563048,
    (1, 60, 1100, 300): 1422088,
    (2, 60, 1094, 1024): 18383024,
    (1, 60, 1094, 1024): 9458456,
    (1, 60, 1094, 300): 1419160,
    (2, 1030, 80, 40): 4004304,
    (1, 1030, 80, 40): 3298536,
    (2, 150, 573, 257): 2826000,
    (1, 150, 573, 257): 1600456,
    (2, 150, 450, 330): 3302000,
    (1, 150, 450, 330): 1882232,
    (2, 127, 165, 100): 643984,
    (1, 127, 165, 100): 390792,
    (1, 127, 165, 99): 389200,
    (2, 128, 165, 100): 667872,
    (1, 128, 165, 100): 413328,
    (1, 128, 165, 99): 411736,
    (1, 60, 80, 0): 50728,
    (3, 60, 80, 0): 132984,
    (1, 60, 80, 1): 51760,
    (3, 60, 80, 1): 134032,
    (1, 1, 80, 40): 16520,
    (2, 1, 80, 40): 30800,
    (1, 1019, 80, 40): 3130440,
    (2, 1019, 80, 40): 3828816,
    (1, 1020, 80, 40): 3140648,
    (2, 1020, 80, 40): 3839696,
    (1, 1021, 80, 40): 3141320,
    (2, 1021, 80, 40): 3841040,
    (1, 1024, 80, 40): 3284456,
    (2, 1024, 80, 40): 3986192,
}


def test_the_layout_holds_every_piece_and_never_exceeds_the_parent_total():
    K = LP.constants()
    sh = shapes()
    _, plans = LP.run([LP.shape_line(i, b, n, cap, rows, lm) for i, (b, n, cap, rows, lm) in enumerate(sh)])
    seen_G = set()
    for (B, n, cap, rows, level_max), p in zip(sh, plans):
        ctx = (B, n, cap, level_max)
        md = max(level_max)
        assert p["maxdim"] == md
        Gmax = (n + K["PTC_MIN"]) // K["PTC_MIN"]  # workgroups of the form with the fewest columns each (column n is the right-hand side)
        assert p["Gmax"] == Gmax == max(f["G"] for f in p["forms"].values()), ctx
        seen_G.add(Gmax)
        stride = -(-Gmax // 16) * 16  # a reader's row of G 16-byte records starts on a 256-byte boundary of the mailbox
        assert p["colld"] >= md + 2, ctx  # a column's rows and its two squared norms, a 16-byte granule each
        # piece -> (bytes the kernels address, alignment of the widest access)
        need = dict(W1=(8 * B * cap * (n + 1), 8), norms0=(8 * B * n, 8), norms1=(8 * B * n, 8), D=(8 * B * n, 8), E=(8 * B * md * md, 8),
                    st0=(K["sizeof(LargeState)"] * B, 8), st1=(K["sizeof(LargeState)"] * B, 8), pos0=(4 * B * (n + 1), 4), pos1=(4 * B * (n + 1), 4),
                    ctl=(K["sizeof(PersistCtl)"], 64), mailbox=(2 * Gmax * stride * K["sizeof(PersistCand)"], 16), colbuf=(2 * Gmax * p["colld"] * 16, 16))
        order = list(p["layout"])
        assert order == list(need), order
        at = 0
        for name in order:  # ascending, no overlap, aligned
            off = p["layout"][name]
            assert off >= at and off % need[name][1] == 0, (ctx, name, off, at)
            at = off + need[name][0]
        assert p["clear"] == (p["layout"]["ctl"], at), ctx  # exactly ctl .. end of the column buffer for the largest G
        assert p["total"] >= at, ctx
        assert p["total"] <= PARENT_TOTAL[(B, n, cap, md)], (ctx, p["total"])
        for (nw, cpw), f in p["forms"].items():  # a form of fewer workgroups clears a prefix of the tail and owns no more than it
            assert f["G"] == (n + nw * cpw) // (nw * cpw) and f["mailbox"] <= need["mailbox"][0] and f["colbuf"] <= need["colbuf"][0], (ctx, nw, cpw)
            assert p["layout"]["ctl"] < f["clear_end"] <= p["total"] and f["clear_end"] == p["layout"]["colbuf"] + f["colbuf"], (ctx, nw, cpw)
            assert f["within"] == int(f["G"] <= K["kPersistMaxG"] and f["lds"] <= K["lexls::kMaxLdsBytes"]), (ctx, nw, cpw)
    assert {K["kPersistMaxG"] - 1, K["kPersistMaxG"], K["kPersistMaxG"] + 1} <= seen_G  # both sides of the form's limit


def test_the_level_plan_covers_the_rows_and_columns_it_is_given():
    K = LP.constants()
    sh = shapes()
    _, plans = LP.run([LP.shape_line(i, b, n, cap, rows, lm) for i, (b, n, cap, rows, lm) in enumerate(sh)])
    taken = set()
    for (B, n, cap, rows, level_max), p in zip(sh, plans):
        assert len(p["levels"]) == len(level_max)
        for k, (lm, lv) in enumerate(zip(level_max, p["levels"])):
            ctx = (n, rows, level_max, k)
            assert lv["gauss"] == int(k + 1 < len(level_max) and rows > 0 and lm > 0), ctx
            assert lv["trsm_cols"] == int(lm <= K["kTrsmColsMax"]), ctx
            taken.add(lv["trsm_cols"])
            if lv["trsm_cols"]:  # a thread per column of the level, whole wavefronts, within the kernel's launch bound
                assert lm <= lv["trsm_block"] <= K["kTrsmColsMax"] and lv["trsm_block"] % 64 == 0 and lv["trsm_block"] - lm < 64, ctx
                per = K["TRB"]
            else:
                assert lv["trsm_block"] == 64
                per = 64
            assert (lv["trsm_grid"] - 1) * per < rows <= lv["trsm_grid"] * per or rows == 0 == lv["trsm_grid"], ctx
            gx, gy = lv["gemm_grid"]
            assert (gx - 1) * K["GBM"] < rows <= gx * K["GBM"] or rows == 0 == gx, ctx
            assert (gy - 1) * K["GBN"] < n + 1 <= gy * K["GBN"], ctx  # n columns and the right-hand side
            ge = lv["level_end_grid"]
            assert (ge - 1) * K["kLevelEndRows"] < rows <= ge * K["kLevelEndRows"] or rows == 0 == ge, ctx
    assert taken == {0, 1}

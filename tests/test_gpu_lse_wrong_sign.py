"""lexls_lse_sensitivity_collect (BatchedLexLSE.sensitivity_collect / wrong_sign): the device form of the collecting overload
ObjectiveSensitivity(ObjIndex, tolW, tolC, ctr_wrong_sign) of the reference (lexlse.h:511-602 around the scan of :866-910), the one
deactivate_first_wrong_sign calls.

Yardstick.  The oracle library computes the multipliers of an objective (oracle.lse_run(..., sens_obj=L)["lam"], the chains of
lexlse.h:611-762); its C interface hands out the deciding overload's verdict only, so the collecting scan itself — comparisons and a sign
flip, no arithmetic — is restated here on the oracle's multipliers, statement for statement as in lexlse.h:891-908 and :575-601: the
objective's own level, the levels above it downwards, then the fixed variables with the reference's quirk (min(dims[0], nVarFixed) entries,
the CONSTRAINT multipliers Lambda[k] against fixed_var_type[k], pushed as ConstraintInfo(-1, k)).  With the scan on, the loop of
lexlsi.h:1072-1083 goes on to the next objective while the set is empty, marks carried along.  Everything is compared exactly: the set, the
marks in both type arrays, LEXLS_ARRAY_LAMBDA and the {non-empty, entries, objective} verdict.  (The end-to-end check against the oracle's
own overload is tests/test_gpu_lsi_first_wrong_sign.py.)"""
import ctypes as C

import numpy as np
import pytest

import postfactor_cases
from lexls_amd import capi, problems as P

pytestmark = pytest.mark.gpu

N, DIMS, BATCH = 14, [4, 5, 5, 4], 8
CAP = sum(DIMS)
LB, UB, EQ, CORRECT = 1, 2, 3, 4
TOLW, TOLC = 1e-8, 1e-12


def inputs(nfixed_of):
    """mixed activation types (LB / UB / EQ) on the rows and on the fixed variables; nfixed_of(b) fixed variables in problem b"""
    lod = P.lse_batch(4100, BATCH, N, DIMS)
    types = np.stack([1 + (P.uniform(4200 + b, CAP) * 3).astype(np.uint8) for b in range(BATCH)])
    types[0, :DIMS[0] + DIMS[1]] = EQ  # the first two objectives of problem 0 have nothing to look at: a scan has to go on
    nfixed = np.array([nfixed_of(b) for b in range(BATCH)], np.uint32)
    idx, val, typ = np.zeros((BATCH, N), np.uint32), np.zeros((BATCH, N)), np.zeros((BATCH, N), np.uint8)
    for b in range(BATCH):
        perm = np.argsort(P.uniform(4300 + b, N))
        idx[b, :nfixed[b]] = perm[:nfixed[b]]
        val[b, :nfixed[b]] = P.normal(4400 + b, N)[:nfixed[b]]
        typ[b, :nfixed[b]] = 1 + (P.uniform(4500 + b, N)[:nfixed[b]] * 3).astype(np.uint8)
    return lod, types, nfixed, idx, val, typ


def reference_collect(oracle, lod, types, nfixed, idx, val, typ, start, scan):
    """the collecting overload on the oracle's multipliers, problem by problem (tests/postfactor_cases.py: the same scan for any shape)"""
    fixed = dict(nfixed=nfixed, fixed_idx=idx, fixed_val=val, fixed_type=typ) if nfixed.any() else {}
    mask, ctr, fix, lam, verdict = postfactor_cases.reference_collect(N, DIMS, lod, DIMS, types, fixed, start, scan)
    return mask, ctr, fix if fixed else typ.copy(), lam, verdict


CASES = {
    "no_fixed": lambda b: 0,
    "fixed_below_dims0": lambda b: 1 + b % 3,        # 1..3 < dims[0] = 4: the quirk scans nVarFixed entries
    "fixed_above_dims0": lambda b: 5 + b % 4,        # 5..8 > dims[0] = 4: the quirk scans dims[0] entries, the rest is never looked at
    "fixed_mixed": lambda b: [0, 2, 4, 6, 9, 1, 5, 3][b],
}


def run_case(hip, oracle, monkeypatch, case, start, scan, policy=None, no_sweep=False):
    lod, types, nfixed, idx, val, typ = inputs(CASES[case])
    want = reference_collect(oracle, lod, types, nfixed, idx, val, typ, start, scan)
    s = hip.BatchedLexLSE(BATCH, N, DIMS)
    if policy is not None:
        s.set_kernel_policy(policy)
    if nfixed.any():
        s.fixVariables(nfixed, idx, val, typ)
    s.setProblem(lod)
    s.setCtrType(types)
    s.factorize_solve()
    s.setSensitivityScan(scan)
    if no_sweep:
        monkeypatch.setenv("LEXLS_SENS_NO_SWEEP", "1")  # (read at every call: sensitivity_kernel serves whatever the shape)
    nonempty, entries, obj = s.sensitivity_collect(start, TOLW, TOLC)
    got = (s.wrong_sign(), s.getCtrType(), s.getFixedType(), s.getWorkspace(), np.stack([nonempty.astype(np.int32), entries, obj], 1))
    maxabs = np.zeros(BATCH)
    capi.check(capi.lib().lexls_lse_get_sensitivity(s._h, None, maxabs.ctypes.data_as(C.POINTER(C.c_double))))
    s.close()
    for name, g, w in zip(("set", "constraint types", "fixed types", "multipliers", "verdict"), got, want):
        np.testing.assert_array_equal(g, w, err_msg=f"{case}: {name}")
    assert not maxabs.any()  # lambda_wrong_sign = 0 on this path (lexlsi.h:1069)
    return want


@pytest.mark.parametrize("scan", [False, True], ids=["one_objective", "scan"])
@pytest.mark.parametrize("case", list(CASES))
def test_collect_on_the_sweep(hip, oracle, monkeypatch, case, scan):
    # (14 variables against 4 + 5 + 5 rows: without fixed variables the first three objectives are met exactly — zero multipliers, nothing to
    # mark or collect — so the single-objective call looks at the last one)
    mask, ctr, fix, _, verdict = run_case(hip, oracle, monkeypatch, case, 0 if scan else 3, scan)
    # the inputs do what they are for: marks, candidates and ignored rows all occur, and a scan stops at different objectives
    assert mask[:, N:].any() and (ctr == CORRECT).any() and (ctr == EQ).any()
    if scan:
        assert verdict[:, 2].max() > 0  # objectives were passed with an empty set
    if scan and case in ("fixed_above_dims0", "fixed_mixed"):
        assert len(set(verdict[:, 2].tolist())) > 1
    if case != "no_fixed":
        assert mask[:, :N].any() or (fix == CORRECT).any()


@pytest.mark.parametrize("scan", [False, True], ids=["one_objective", "scan"])
@pytest.mark.parametrize("case", ["no_fixed", "fixed_mixed"])
def test_collect_on_sensitivity_kernel(hip, oracle, monkeypatch, case, scan):
    """the per-objective kernel of lse_postfactor.hip (the shapes the sweep does not serve): forced with LEXLS_SENS_NO_SWEEP"""
    run_case(hip, oracle, monkeypatch, case, 0 if scan else 3, scan, no_sweep=True)


def test_collect_under_kernel_policy_1(hip, oracle, monkeypatch):
    """the factor of the generic l-QR kernel (policy 1) under the collecting search"""
    run_case(hip, oracle, monkeypatch, "fixed_mixed", 0, True, policy=1)


def test_per_problem_objectives_and_skips(hip, oracle):
    """objective indices per problem, a negative one skips the problem: its verdict is {0, -1, -2}, as lexls_lse_sensitivity's"""
    lod, types, nfixed, idx, val, typ = inputs(CASES["fixed_mixed"])
    s = hip.BatchedLexLSE(BATCH, N, DIMS)
    s.fixVariables(nfixed, idx, val, typ)
    s.setProblem(lod)
    s.setCtrType(types)
    s.factorize_solve()
    oi = np.array([3, -1, 2, 1, 0, -1, 3, 2], np.int32)
    nonempty, entries, obj = s.sensitivity_collect(oi, TOLW, TOLC)
    mask = s.wrong_sign()
    s.close()
    for L in range(len(DIMS)):
        want = reference_collect(oracle, lod, types, nfixed, idx, val, typ, L, False)
        for b in np.flatnonzero(oi == L):
            np.testing.assert_array_equal(mask[b], want[0][b])
            assert (int(nonempty[b]), int(entries[b]), int(obj[b])) == tuple(want[4][b])
    for b in np.flatnonzero(oi < 0):
        assert (int(nonempty[b]), int(entries[b]), int(obj[b])) == (0, -1, -2)

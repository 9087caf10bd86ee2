"""Small batches that take the ZERO-COPY input path of LexLSE (lexls_lse_set_problem_device: a caller-owned device pointer, bound as it is)
through every kernel family that reads `in`.  tests/test_gpu_device_input.py binds each of them at a 16-byte and at an 8-byte aligned base and
holds the results to the oracle; tests/test_device_input_cases.py asserts on the CPU, from the oracle and the planner alone, that each case has
the ranks and reaches the kernel this text says.  Plain data: no GPU, no torch.

Why the base matters: query_of (lexls_capi.hip) classifies the pointer as 16 / 8 / less, and only lqr_qtol's uniform form and lqr_mfma read that
field (they give way to the bit-exact kernel below 16).  The bit-exact kernels choose between 16-byte and 8-byte level loads from offsets
RELATIVE to the base (lqr_quad_impl.h: ((F + pc * cap) & 1) == 0; lqr_lwave_impl.h: ((cap | Frow) & 1) == 0), so at an 8-byte base their
16-byte loads go to addresses that are 8 mod 16.  A problem is cap x (nVar + 1) doubles: where that product is odd (`oddld`, 39 x 31)
consecutive problems alternate between the two alignments whatever the base.

Data: P.lse_batch(seed, batch, n, caps), batches of 5 - 13 (a four-per-wavefront tail exists; the large path: one problem).  `deficient`: the
last two problems are P.rank_deficient_problem with the ranks given (exact dependences on the levels above).  `per_problem`: the ragged
construction of tests/test_gpu_parity.py::test_ragged_batch — problem b's rows packed level after level, zeros behind them.  `fixed`: fixed
variables dealt round the batch (0, 1, 2, 3, ... of them, random indices and values).  `reg`: Tikhonov (type 1), one factor per level.

MEASURED (oracle alone, `python tests/device_input_cases.py`; held by tests/test_device_input_cases.py): the kernel is the one at a 16-byte
base, ranks = the levels' ranks of problem 0, full / deficient k = no problem / k problems with a level below the rank its rows and the columns
left allow:
    q1_x       n=12  [4,4,4]           batch 9  policy 4  keep 0 lqr_quad<1,12>                       ranks [4,4,4]          full
    q1_f       n=12  [4,4,4]           batch 9  policy 4  keep 1 lqr_quad<1,12,factor>                ranks [4,4,4]          full
    q2_x       n=20  [12,12,12]        batch 13 policy 4  keep 0 lqr_quad<2,12>                       ranks [12,8,0]         deficient 2
    q2_f       n=20  [12,12,12]        batch 13 policy 4  keep 1 lqr_quad<2,12,factor>                ranks [12,8,0]         deficient 2
    q3_x       n=33  [11,7,12,3]       batch 7  policy 4  keep 0 lqr_quad<3,12>                       ranks [11,7,12,3]      full
    q3_f       n=33  [11,7,12,3]       batch 7  policy 4  keep 1 lqr_quad<3,12,factor>                ranks [11,7,12,3]      full
    q3s7_x     n=40  [12,12,12,12,12]  batch 11 policy 4  keep 0 lqr_quad<3,12,shift 7>               ranks [12,12,12,4,0]   deficient 2
    q3s7_f     n=40  [12,12,12,12,12]  batch 11 policy 4  keep 1 lqr_quad<3,12,shift 7,factor>        ranks [12,12,12,4,0]   deficient 2
    q3s7_xF    n=40  [12,12,12,12,12]  batch 11 policy 4  keep 0 lqr_quad<3,12,shift 7,fixed>         ranks [12,12,12,4,0]   deficient 2
    q4_x       n=55  [16,8,16,16]      batch 5  policy 4  keep 0 lqr_quad<4,16>                       ranks [16,8,16,15]     full
    q4_f       n=55  [16,8,16,16]      batch 5  policy 4  keep 1 lqr_quad<4,16,factor>                ranks [16,8,16,15]     full
    lw41       n=30  [9,12,5]          batch 9  policy 3  keep 1 lqr_lwave<41,12>                     ranks [9,12,5]         deficient 2
    lw41e      n=40  [12,12,12,12,12]  batch 6  policy 3  keep 1 lqr_lwave<41,12,exact>               ranks [12,12,12,4,0]   full
    w41e       n=40  [12,12,12,12,12]  batch 6  policy 2  keep 1 lqr_wave<41,12,exact>                ranks [12,12,12,4,0]   full
    w41F       n=30  [9,12,5]          batch 9  policy 2  keep 1 lqr_wave<41,12>                      ranks [9,12,5]         deficient 2
    w64        n=63  [16,16,16,16]     batch 5  policy 2  keep 1 lqr_wave<64,16>                      ranks [16,16,16,15]    full
    wreg       n=20  [6,5,5,6]         batch 7  policy 0  keep 1 lqr_wave<41,12,regularized>          ranks [6,5,5,4]        full
    g64        n=40  [12,12,12,12,12]  batch 6  policy 1  keep 1 lqr_generic<64,lds>                  ranks [12,12,12,4,0]   full
    g256       n=100 [30,30,30,30]     batch 5  policy 0  keep 1 lqr_generic<256,lds>                 ranks [30,30,30,10]    full
    large_b    n=100 [115,115]         batch 1  policy 5  keep 1 lqr_large<multi-launch>              ranks [100,0]          full
    large_t    n=100 [115,115]         batch 1  policy 0  keep 1 lqr_large<step-per-pivot,mfma>       ranks [100,0]          full
    ragged     n=40  [12,12,12,12,12]  batch 13 policy 10 keep 0 lqr_qtol<3,12,shift 7,ragged>        ranks [0,3,6,9,12]     per-problem dims
    t_auto     n=40  [12,12,12,12,12]  batch 11 policy 0  keep 0 lqr_qtol<3,12,shift 7>               ranks [12,12,12,4,0]   deficient 2 (8-byte base: lqr_quad<3,12,shift 7>)
    t_qtol     n=40  [12,12,12,12,12]  batch 11 policy 6  keep 0 lqr_qtol<3,12,shift 7>               ranks [12,12,12,4,0]   deficient 2 (8-byte base: lqr_quad<3,12,shift 7>)
    t_mfma     n=40  [12,12,12,12,12]  batch 11 policy 7  keep 0 lqr_mfma<32,12,n40>                  ranks [12,12,12,4,0]   deficient 2 (8-byte base: lqr_quad<3,12,shift 7>)
    oddld_w    n=30  [14,9,16]         batch 8  policy 2  keep 1 lqr_wave<64,16>                      ranks [14,9,7]         deficient 2
    oddld_q    n=30  [14,9,16]         batch 8  policy 4  keep 0 lqr_quad<4,16>                       ranks [14,9,7]         deficient 2

Every shape is expressed to tests/dispatch_plan_check.cpp (query lines of scripts/record_dispatch_table.py, which takes an entry's own
capacities and dimensions for that): no kernel name is asserted on the GPU alone.
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from lexls_amd import problems as P  # noqa: E402

IK = [12] * 5
QS7 = "lqr_quad<3,12,shift 7>"
# contract: "B" bit for bit; "T" permutation / ranks / first columns exact, x within 1e-10 max(1, |x|inf); "L" the step-per-pivot large path
# (assert_factor_close of tests/test_gpu_parity.py).  kernel8: the name at an 8-byte aligned base where it differs — the bit-exact kernel the
# (T) kernels give way to, whose results are then held bit for bit
# deficient: ranks of the last two problems' construction (rank_deficient_problem); fixed / reg: flags; ragged: per-problem dimensions
CASES = {
    "q1_x": dict(n=12, caps=[4] * 3, batch=9, seed=20290001, policy=4, keep=0, kernel="lqr_quad<1,12>"),
    "q1_f": dict(n=12, caps=[4] * 3, batch=9, seed=20290001, policy=4, keep=1, kernel="lqr_quad<1,12,factor>"),
    "q2_x": dict(n=20, caps=[12] * 3, batch=13, seed=20290002, policy=4, keep=0, kernel="lqr_quad<2,12>", deficient=[7, 5, 3]),
    "q2_f": dict(n=20, caps=[12] * 3, batch=13, seed=20290002, policy=4, keep=1, kernel="lqr_quad<2,12,factor>", deficient=[7, 5, 3]),
    "q3_x": dict(n=33, caps=[11, 7, 12, 3], batch=7, seed=20290003, policy=4, keep=0, kernel="lqr_quad<3,12>"),
    "q3_f": dict(n=33, caps=[11, 7, 12, 3], batch=7, seed=20290003, policy=4, keep=1, kernel="lqr_quad<3,12,factor>"),
    "q3s7_x": dict(n=40, caps=IK, batch=11, seed=20290004, policy=4, keep=0, kernel=QS7, deficient=[7, 12, 3, 9, 2]),
    "q3s7_f": dict(n=40, caps=IK, batch=11, seed=20290004, policy=4, keep=1, kernel="lqr_quad<3,12,shift 7,factor>", deficient=[7, 12, 3, 9, 2]),
    "q3s7_xF": dict(n=40, caps=IK, batch=11, seed=20290004, policy=4, keep=0, kernel="lqr_quad<3,12,shift 7,fixed>", deficient=[7, 12, 3, 9, 2], fixed=1),
    "q4_x": dict(n=55, caps=[16, 8, 16, 16], batch=5, seed=20290005, policy=4, keep=0, kernel="lqr_quad<4,16>"),
    "q4_f": dict(n=55, caps=[16, 8, 16, 16], batch=5, seed=20290005, policy=4, keep=1, kernel="lqr_quad<4,16,factor>"),
    "lw41": dict(n=30, caps=[9, 12, 5], batch=9, seed=20290006, policy=3, keep=1, kernel="lqr_lwave<41,12>", deficient=[5, 9, 2]),
    "lw41e": dict(n=40, caps=IK, batch=6, seed=20290007, policy=3, keep=1, kernel="lqr_lwave<41,12,exact>"),
    "w41e": dict(n=40, caps=IK, batch=6, seed=20290007, policy=2, keep=1, kernel="lqr_wave<41,12,exact>"),
    "w41F": dict(n=30, caps=[9, 12, 5], batch=9, seed=20290006, policy=2, keep=1, kernel="lqr_wave<41,12>", deficient=[5, 9, 2], fixed=1),
    "w64": dict(n=63, caps=[16] * 4, batch=5, seed=20290008, policy=2, keep=1, kernel="lqr_wave<64,16>"),
    "wreg": dict(n=20, caps=[6, 5, 5, 6], batch=7, seed=20290009, policy=0, keep=1, kernel="lqr_wave<41,12,regularized>", reg=1),
    "g64": dict(n=40, caps=IK, batch=6, seed=20290007, policy=1, keep=1, kernel="lqr_generic<64,lds>"),
    "g256": dict(n=100, caps=[30] * 4, batch=5, seed=20290010, policy=0, keep=1, kernel="lqr_generic<256,lds>"),
    "large_b": dict(n=100, caps=[115, 115], batch=1, seed=20290011, policy=5, keep=1, kernel="lqr_large<multi-launch>"),
    "large_t": dict(n=100, caps=[115, 115], batch=1, seed=20290011, policy=0, keep=1, kernel="lqr_large<step-per-pivot,mfma>", contract="L"),
    "ragged": dict(n=40, caps=IK, batch=13, seed=20290012, policy=10, keep=0, kernel="lqr_qtol<3,12,shift 7,ragged>", contract="T", ragged=1),
    "t_auto": dict(n=40, caps=IK, batch=11, seed=20290004, policy=0, keep=0, kernel="lqr_qtol<3,12,shift 7>", kernel8=QS7, contract="T", deficient=[7, 12, 3, 9, 2]),
    "t_qtol": dict(n=40, caps=IK, batch=11, seed=20290004, policy=6, keep=0, kernel="lqr_qtol<3,12,shift 7>", kernel8=QS7, contract="T", deficient=[7, 12, 3, 9, 2]),
    "t_mfma": dict(n=40, caps=IK, batch=11, seed=20290004, policy=7, keep=0, kernel="lqr_mfma<32,12,n40>", kernel8=QS7, contract="T", deficient=[7, 12, 3, 9, 2]),
    "oddld_w": dict(n=30, caps=[14, 9, 16], batch=8, seed=20290013, policy=2, keep=1, kernel="lqr_wave<64,16>", deficient=[9, 9, 5]),
    "oddld_q": dict(n=30, caps=[14, 9, 16], batch=8, seed=20290013, policy=4, keep=0, kernel="lqr_quad<4,16>", deficient=[9, 9, 5]),
}
REG_FACTORS = [0.4, 0.15, 0.3, 0.05]  # `wreg`
BIT_EXACT = tuple(nm for nm, c in CASES.items() if c.get("contract", "B") == "B")
# the consumers behind the factorization (get_v, ObjectiveSensitivity, multipliers, least-norm solve, factorize + solve) run over these
CONSUMER_CASES = ("w41e", "q3s7_f", "g64")


def kernel_at(name, align):
    c = CASES[name]
    return c.get("kernel8", c["kernel"]) if align == 8 else c["kernel"]


def contract_at(name, align):
    """what the results at this alignment are held to: a (T) kernel that gave way leaves a bit-exact kernel behind"""
    c = CASES[name]
    return "B" if (align == 8 and "kernel8" in c) else c.get("contract", "B")


def ragged_dims(batch, nobj):
    """per-problem dimensions 0 ... 12: problem b's level k has 3 (b + k) mod 13 rows — every size, empty levels, a full one next to them"""
    return np.array([[(3 * (b + k)) % 13 for k in range(nobj)] for b in range(batch)], np.uint32)


def draw(name):
    """the inputs of a case: dict(name, n, caps, lod (batch, n + 1, cap), dims (batch, nObj), fixed (keyword arguments of oracle.lse_run, {}
    without fixed variables), types (batch, cap) activation types for the consumers, reg (type, factors) or None)"""
    c = CASES[name]
    n, caps, B, seed = c["n"], list(c["caps"]), c["batch"], c["seed"]
    cap = sum(caps)
    dims = np.tile(np.asarray(caps, np.uint32), (B, 1))
    if c.get("ragged"):
        dims = ragged_dims(B, len(caps))
        lod = np.zeros((B, n + 1, cap))
        for b in range(B):
            m = int(dims[b].sum())
            lod[b, :, :m] = P.lse_problem(seed + b, n, dims[b])
    else:
        lod = P.lse_batch(seed, B, n, caps)
        if c.get("deficient"):
            for b in (B - 2, B - 1):
                lod[b] = P.rank_deficient_problem(seed + 1000 + b, n, caps, c["deficient"])
    fixed = {}
    if c.get("fixed"):
        nfixed = (np.arange(B) % 5).astype(np.uint32)
        idx, val = np.zeros((B, n), np.uint32), np.zeros((B, n))
        typ = np.full((B, n), 2, np.uint8)
        for b in range(B):
            nf = int(nfixed[b])
            idx[b, :nf] = np.argsort(P.uniform(seed + 300000 + b, n))[:nf]
            val[b, :nf] = P.normal(seed + 400000 + b, n)[:nf]
        fixed = dict(nfixed=nfixed, fixed_idx=idx, fixed_val=val, fixed_type=typ)
    types = np.stack([1 + (P.uniform(seed + 500000 + b, cap) * 3).astype(np.uint8) for b in range(B)])  # LB / UB / EQ
    reg = (c["reg"], np.asarray(REG_FACTORS[:len(caps)])) if c.get("reg") else None
    return dict(name=name, n=n, caps=caps, lod=np.ascontiguousarray(lod), dims=dims, fixed=fixed, types=types, reg=reg, policy=c["policy"], keep=bool(c["keep"]))


def reference(case, oracle, lod=None):
    """the oracle on the case (or on other data of its shape): everything the GPU test compares"""
    kw = dict(case["fixed"])
    if case["reg"]:
        kw.update(reg_type=case["reg"][0], reg_factors=case["reg"][1])
    return oracle.lse_run(case["lod"] if lod is None else lod, case["dims"], case["n"], maxdim=np.asarray(case["caps"], np.uint32), **kw)


def consumer_reference(case, oracle):
    """per level k the oracle's ObjectiveSensitivity(k) from the case's activation types (verdict, largest multiplier, [lambda_fixed; lambda],
    marks), the multipliers of every level stacked as multipliers() returns them, and the least-norm solution of solveLeastNorm_1"""
    n, caps = case["n"], np.asarray(case["caps"], np.uint32)
    out = dict(sens=[], maxabs=[], lam=[], marks=[])
    for k in range(len(caps)):
        r = oracle.lse_run(case["lod"], case["dims"], n, maxdim=caps, ctr_type=case["types"], sens_obj=k, **case["fixed"])
        out["sens"].append(r["sens"]), out["maxabs"].append(r["maxabs"]), out["lam"].append(r["lam"]), out["marks"].append(r["ctr_type_out"])
    out["mult"] = np.stack(out["lam"], axis=1)
    out["ln1"] = oracle.lse_run(case["lod"], case["dims"], n, maxdim=caps, solve_option=1, **case["fixed"])["x"]
    return out


def _freeze(tree):
    for v in tree.values() if isinstance(tree, dict) else tree:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)  # shared among the tests: nobody changes it
        elif isinstance(v, (dict, list)):
            _freeze(v)


@functools.lru_cache(maxsize=None)
def build(name):
    """the case with ref = the oracle's results, computed once and shared (read-only); consumers: consumer_reference for CONSUMER_CASES"""
    from oracle import oracle_ctypes as oracle
    case = draw(name)
    case["ref"] = reference(case, oracle)
    if name in CONSUMER_CASES:
        case["consumers"] = consumer_reference(case, oracle)
    _freeze(case)
    return case


@functools.lru_cache(maxsize=None)
def other_data(name, which=1):
    """a second (third, ...) batch of the case's shape with its oracle results: what a rebound or overwritten buffer holds"""
    from oracle import oracle_ctypes as oracle
    case = build(name)
    lod = P.lse_batch(CASES[name]["seed"] + 7000 * which, CASES[name]["batch"], case["n"], case["caps"])
    out = dict(lod=lod, ref=reference(case, oracle, lod))
    _freeze(out)
    return out


def deficient_problems(case):
    """problems with a level whose rank is below what its rows and the columns left allow"""
    ref, n = case["ref"], case["n"]
    return [b for b in range(len(case["lod"]))
            if any(int(ref["rank"][b, k]) < min(int(case["dims"][b, k]), n - int(ref["fcol"][b, k])) for k in range(len(case["caps"])))]


def summary(case):
    c = CASES[case["name"]]
    short = deficient_problems(case)
    what = "per-problem dims" if c.get("ragged") else (f"deficient {len(short)}" if short else "full")
    line = (f"    {case['name']:<10} n={case['n']:<3} {str(case['caps']).replace(' ', ''):<17} batch {len(case['lod']):<2} policy {c['policy']:<2} keep {c['keep']} "
            f"{c['kernel']:<36} ranks {str(case['ref']['rank'][0].tolist()).replace(' ', ''):<16} {what}")
    return line + (f" (8-byte base: {c['kernel8']})" if "kernel8" in c else "")


if __name__ == "__main__":
    for nm in CASES:
        print(summary(build(nm)))

"""The zero-copy input path of LexLSE — lexls_lse_set_problem_device: a caller-owned device pointer, often offset into a larger buffer, often
on a caller-owned stream — against the oracle, on the cases of tests/device_input_cases.py (tests/test_device_input_cases.py holds their ranks
and kernels on the CPU).  Every other GPU test of the equality solver hands its problem over with setProblem: a copy into the handle's own
256-byte aligned allocation on the default stream.  bench.py and every integrator of INTEGRATION.md come this way instead.

a. values at a 16-byte and at an 8-byte aligned base, every kernel family; b. the consumers behind the factorization over a bound pointer;
c. the input (and 16 sentinel doubles on either side of it) bit-identical after every run; d. a pointer that is no multiple of 8 refused, the
handle left as it was; e. rebinding: rotation, two handles on two halves of one buffer, contents overwritten in place; f. a user stream
ordered by nothing but the stream.  torch appears for buffers and streams only.  Nothing here is a timing test and no new number appears:
bitwise equality, or the project's contract (T) of 1e-10 where a case's kernel is a tolerance-contract one."""
import numpy as np
import pytest
import torch  # (before the HIP library loads: one process, one HIP runtime)

import device_input_cases as D
from factor_checks import assert_factor_equal
from lexls_amd import problems as P
from test_gpu_parity import assert_factor_close

pytestmark = pytest.mark.gpu

PAD = 16  # sentinel doubles in front of and behind the data
TOL = 1e-10  # contract (T), include/lexls_hip.h


class Placed:
    """`lod` in a torch.float64 device tensor at element offset 0 (16-byte aligned data) or 1 (8 mod 16), NaN sentinels round it"""

    def __init__(self, lod, align):
        off = {16: 0, 8: 1}[align]
        host = np.full(PAD + off + lod.size + PAD, np.nan)
        host[PAD + off:PAD + off + lod.size] = np.ascontiguousarray(lod, np.float64).reshape(-1)
        self.t = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        assert self.t.data_ptr() % 16 == 0
        self.first, self.count = PAD + off, lod.size
        self.ptr = self.t.data_ptr() + 8 * self.first
        assert self.ptr % 16 == (0 if align == 16 else 8)
        self.bits = host.view(np.int64).copy()

    def data(self):
        """the tensor's view of the problem data (what a caller overwrites in place)"""
        return self.t[self.first:self.first + self.count]

    def expect(self, lod):
        """from now on the buffer is meant to hold `lod`"""
        self.bits[self.first:self.first + self.count] = np.ascontiguousarray(lod, np.float64).reshape(-1).view(np.int64)

    def assert_untouched(self):
        torch.cuda.synchronize()
        np.testing.assert_array_equal(self.t.cpu().numpy().view(np.int64), self.bits, err_msg="the bound buffer (sentinels included) was written")


def on_device(lod):
    """a flat device copy of a host array (the shared references are read-only: torch wants a writable source)"""
    return torch.from_numpy(np.array(lod, np.float64).reshape(-1)).cuda()


def handle(hip, case, policy=None, batch=None):
    B = len(case["lod"]) if batch is None else batch
    s = hip.BatchedLexLSE(B, case["n"], case["caps"])
    s.set_kernel_policy(case["policy"] if policy is None else policy)
    if (case["dims"] != np.asarray(case["caps"], np.uint32)).any():
        s.setObjDim(case["dims"][:B])
    if case["reg"]:
        s.setRegularization(case["reg"][0], case["reg"][1])
    f = case["fixed"]
    if f:
        s.fixVariables(f["nfixed"][:B], f["fixed_idx"][:B], f["fixed_val"][:B], f["fixed_type"][:B])
    return s


def check_pivots(s, ref):
    r, fc, tr = s.getRanks()
    np.testing.assert_array_equal(r, ref["rank"])
    np.testing.assert_array_equal(fc, ref["fcol"])
    np.testing.assert_array_equal(tr, ref["totalrank"])
    np.testing.assert_array_equal(s.get_column_permutations(), ref["perm"])


def check_values(s, case, ref, contract, keep):
    """the results of the last factorize_solve against the oracle's under the case's contract; returns x"""
    x = s.get_x()
    if contract == "B":
        if keep:
            assert_factor_equal(s, ref, case["dims"], case["n"])  # ranks, first columns, permutation, Householder scalars, factor: bit for bit
        check_pivots(s, ref)
        np.testing.assert_array_equal(x, ref["x"])
    elif contract == "L":
        assert_factor_close(s, ref, case["dims"], case["n"])
    else:
        check_pivots(s, ref)
        assert np.isfinite(x).all()
        err = float(np.abs(x - ref["x"]).max())
        print(f"{case['name']} {s.last_kernel()}: max|x - x_oracle| = {err:.3e}")
        assert err <= TOL * max(1.0, float(np.abs(ref["x"]).max()))
    return x


# ---- a. values at both alignments, c. input untouched ---------------------------------------------------------------------------------
@pytest.mark.parametrize("align", [16, 8])
@pytest.mark.parametrize("name", list(D.CASES))
def test_a_values_at_both_alignments(hip, name, align):
    case = D.build(name)
    s = handle(hip, case)
    buf = Placed(case["lod"], align)
    s.setProblemDevice(buf.ptr)
    s.factorize_solve(keep_factor=case["keep"])
    assert s.last_kernel() == D.kernel_at(name, align)
    check_values(s, case, case["ref"], D.contract_at(name, align), case["keep"])
    buf.assert_untouched()
    s.close()


def test_a_ragged_qtol_gives_the_same_bits_at_both_alignments(hip):
    """the same kernel on the same data: where the base stands must not show in x"""
    case, xs = D.build("ragged"), []
    for align in (16, 8):
        s = handle(hip, case)
        buf = Placed(case["lod"], align)
        s.setProblemDevice(buf.ptr)
        s.factorize_solve(keep_factor=False)
        assert s.last_kernel() == "lqr_qtol<3,12,shift 7,ragged>"
        xs.append(s.get_x())
        buf.assert_untouched()
        s.close()
    np.testing.assert_array_equal(xs[0], xs[1])


# ---- b. the consumers behind the factorization read the bound pointer again -----------------------------------------------------------
@pytest.mark.parametrize("name", D.CONSUMER_CASES)
def test_b_consumers_over_a_bound_pointer(hip, name):
    """get_v, ObjectiveSensitivity at every level, multipliers(), solveLeastNorm_1, then factorize() + solve() apart, all at the 8-byte base:
    as tests/test_gpu_parity.py and tests/test_gpu_postfactor.py hold them for host input"""
    case = D.build(name)
    ref, want = case["ref"], case["consumers"]
    s = handle(hip, case)
    buf = Placed(case["lod"], 8)
    s.setProblemDevice(buf.ptr)
    s.setCtrType(case["types"])
    s.factorize_solve(keep_factor=True)
    assert s.last_kernel() == D.kernel_at(name, 8)
    np.testing.assert_array_equal(s.get_x(), ref["x"])
    m = case["dims"].sum(axis=1)
    v = s.get_v()
    for b in range(len(m)):
        np.testing.assert_array_equal(v[b, :m[b]], ref["v"][b, :m[b]], err_msg=f"v of problem {b}")
    found_any = False
    for k in range(len(case["caps"])):
        s.setCtrType(case["types"])  # every oracle result starts from the types as given; the handle keeps the marks of the call before
        found, ctr, obj, maxabs = s.ObjectiveSensitivity(k)
        w = want["sens"][k]
        np.testing.assert_array_equal(found.astype(np.int32), w[:, 0], err_msg=f"found, level {k}")
        np.testing.assert_array_equal(np.where(found, ctr, 0), np.where(found, w[:, 1], 0), err_msg=f"ctr, level {k}")
        np.testing.assert_array_equal(np.where(found, obj, 0), np.where(found, w[:, 2], 0), err_msg=f"obj, level {k}")
        np.testing.assert_array_equal(maxabs, want["maxabs"][k], err_msg=f"maxabs, level {k}")
        np.testing.assert_array_equal(s.getWorkspace(), want["lam"][k], err_msg=f"multipliers, level {k}")
        np.testing.assert_array_equal(s.getCtrType(), want["marks"][k], err_msg=f"marks, level {k}")
        found_any = found_any or bool(found.any())
    assert found_any and (want["mult"] != 0.0).any()  # (not a comparison of zeros)
    s.setCtrType(case["types"])
    np.testing.assert_array_equal(s.multipliers(), want["mult"])
    s.solveLeastNorm_1()
    np.testing.assert_array_equal(s.get_x(), want["ln1"])
    buf.assert_untouched()
    s.factorize()
    s.solve()
    np.testing.assert_array_equal(s.get_x(), ref["x"])
    assert_factor_equal(s, ref, case["dims"], case["n"])
    buf.assert_untouched()
    s.close()


# ---- d. a pointer that is not a multiple of 8 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["q3s7_x", "w41e"])
def test_d_misaligned_pointer_refused(hip, name):
    """no kernel is launched on such a pointer: a fresh handle stays without input, a bound one keeps its problem and its factor"""
    case = D.build(name)
    buf = Placed(case["lod"], 16)
    fresh = handle(hip, case)
    for shift in (4, 1, 12):
        with pytest.raises(hip.LexlsError, match="multiple of 8"):
            fresh.setProblemDevice(buf.ptr + shift)
    assert fresh.last_kernel() == ""
    with pytest.raises(hip.LexlsError, match="no problem data"):
        fresh.factorize_solve(keep_factor=case["keep"])
    assert fresh.last_kernel() == ""
    fresh.close()
    s = handle(hip, case)
    s.setProblemDevice(buf.ptr)
    s.factorize_solve(keep_factor=case["keep"])
    other = Placed(D.other_data(name)["lod"], 16)
    with pytest.raises(hip.LexlsError, match="multiple of 8"):
        s.setProblemDevice(other.ptr + 4)
    if case["keep"]:  # the handle as it was: the kept factor is still served
        assert_factor_equal(s, case["ref"], case["dims"], case["n"])
        s.solve()
    np.testing.assert_array_equal(s.get_x(), case["ref"]["x"])
    s.factorize_solve(keep_factor=case["keep"])  # the previously bound problem is still the one solved
    assert s.last_kernel() == D.kernel_at(name, 16)
    np.testing.assert_array_equal(s.get_x(), case["ref"]["x"])
    buf.assert_untouched()
    other.assert_untouched()
    s.close()


# ---- e. rebinding ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w41e", "q3s7_x"])
def test_e_rotation_between_two_buffers(hip, name):
    """(i) one handle, buffers A, B, A as bench.py rotates its resident batches (B at the 8-byte base): every x is the oracle's for the buffer
    bound at the time; straight after a rebind the factor of the buffer before is gone.  The lqr_wave case keeps its factor with prefix reuse
    on: the state a factorization leaves for the next one must not carry levels of the other buffer over"""
    case = D.build(name)
    a, b = dict(lod=case["lod"], ref=case["ref"]), D.other_data(name)
    s = handle(hip, case)
    if case["keep"]:
        s.set_prefix_reuse(True)
    bufs = [Placed(a["lod"], 16), Placed(b["lod"], 8)]
    for which in (0, 1, 0):
        s.setProblemDevice(bufs[which].ptr)
        with pytest.raises(hip.LexlsError):
            s.solve()  # factor dropped
        with pytest.raises(hip.LexlsError):
            s.get_lexqr()
        s.factorize_solve(keep_factor=case["keep"])
        assert s.last_kernel() == D.kernel_at(name, 16)
        check_values(s, case, (a, b)[which]["ref"], "B", case["keep"])
        if case["keep"]:
            assert s.prefix_reuse_ready()
    for buf in bufs:
        buf.assert_untouched()
    s.close()


@pytest.mark.parametrize("align", [16, 8])
@pytest.mark.parametrize("policy,keep,kernel", [(4, False, "lqr_quad<4,16>"), (2, True, "lqr_wave<64,16>")])
def test_e_two_handles_on_two_halves_of_one_buffer(hip, oracle, policy, keep, kernel, align):
    """(ii) two handles of batch 6 on the halves of one batch-12 buffer, the second half's pointer base + 6 cap (n + 1) 8.  That offset is
    48 cap (n + 1) bytes, a multiple of 16 for every shape, so it cannot be 8 mod 16 by itself: the shape is the one whose problems are an odd
    number of doubles (n = 30, [14,9,16]: 39 x 31; problems alternate between the two alignments inside each half) and the whole arrangement
    runs at a 16-byte and at an 8-byte base, where both halves are 8 mod 16"""
    case = D.build("oddld_q")
    n, caps = case["n"], case["caps"]
    lod = P.lse_batch(20290100, 12, n, caps)
    ref = oracle.lse_run(lod, caps, n)
    buf = Placed(lod, align)
    half = 6 * sum(caps) * (n + 1) * 8
    hs = []
    for i in range(2):
        s = handle(hip, case, policy=policy, batch=6)
        s.setProblemDevice(buf.ptr + i * half)
        hs.append(s)
    for s in hs:
        s.factorize_solve(keep_factor=keep)
    for i, s in enumerate(hs):
        assert s.last_kernel() == kernel
        check_values(s, dict(case, dims=case["dims"][:6]), {k: v[6 * i:6 * i + 6] for k, v in ref.items()}, "B", keep)
        s.close()
    buf.assert_untouched()


@pytest.mark.parametrize("name", ["q2_x", "w41F"])
def test_e_contents_overwritten_in_place(hip, name):
    """(iii) the same pointer, new contents written by torch, setProblemDevice again: the new data's result (and the old factor is gone)"""
    case, new = D.build(name), D.other_data(name)
    s = handle(hip, case)
    buf = Placed(case["lod"], 8)
    s.setProblemDevice(buf.ptr)
    s.factorize_solve(keep_factor=case["keep"])
    check_values(s, case, case["ref"], "B", case["keep"])
    buf.data().copy_(on_device(new["lod"]))
    torch.cuda.synchronize()
    buf.expect(new["lod"])
    s.setProblemDevice(buf.ptr)
    with pytest.raises(hip.LexlsError):
        s.get_lexqr()
    s.factorize_solve(keep_factor=case["keep"])
    assert s.last_kernel() == D.kernel_at(name, 8)
    check_values(s, case, new["ref"], "B", case["keep"])
    buf.assert_untouched()
    s.close()


# ---- f. a user stream, ordered by the stream only -------------------------------------------------------------------------------------
def keep_busy(scratch, rounds=100):
    """elementwise passes over a large tensor: some tens of milliseconds of work in front of whatever is enqueued next on the current stream"""
    for _ in range(rounds):
        scratch.mul_(1.0000001)


@pytest.fixture(scope="module")
def scratch():
    t = torch.ones(1 << 26, dtype=torch.float64, device="cuda")  # 512 MB: a pass reads and writes 1 GB
    yield t
    del t


@pytest.mark.parametrize("name", ["q3s7_x", "w41F", "g64"])
def test_f_input_written_on_the_user_stream_just_before_the_solve(hip, scratch, name):
    """the bound buffer holds Old; on the handle's stream, behind tens of milliseconds of other work, New is copied over it and the solve is
    enqueued at once, with no host synchronisation in between: x is New's.  For the handle's FIRST factorization (lexls_lse_create clears its
    round slabs on the null stream, which does not order torch's non-blocking streams: the fixed variables of `w41F` travel through that slab)
    and for a later one"""
    case = D.build(name)
    old = dict(lod=case["lod"], ref=case["ref"])
    rounds = [D.other_data(name, 1), D.other_data(name, 2)]
    assert (np.abs(rounds[0]["ref"]["x"] - old["ref"]["x"]).max(axis=1) > 1e-3).all()  # a solve that saw Old cannot pass
    assert (np.abs(rounds[1]["ref"]["x"] - rounds[0]["ref"]["x"]).max(axis=1) > 1e-3).all()
    new_dev = [on_device(r["lod"]) for r in rounds]
    buf = Placed(old["lod"], 8)
    torch.cuda.synchronize()  # uploads done, on the default stream
    st = torch.cuda.Stream()
    s = handle(hip, case)  # (its setters wait for the handle's stream: all of them come before the stream is made busy)
    s.set_stream(st.cuda_stream)
    s.setProblemDevice(buf.ptr)
    for r, dev in zip(rounds, new_dev):
        with torch.cuda.stream(st):
            keep_busy(scratch)
            buf.data().copy_(dev, non_blocking=True)
            done = torch.cuda.Event()
            done.record(st)
        s.factorize_solve(keep_factor=case["keep"])
        print(f"{name}: the stream was {'still busy' if not done.query() else 'idle'} when factorize_solve returned")
        buf.expect(r["lod"])
        assert s.last_kernel() == D.kernel_at(name, 8)
        check_values(s, case, r["ref"], "B", case["keep"])  # (the getters wait for the handle's stream)
        buf.assert_untouched()
    s.close()


def test_f_two_handles_on_two_streams_interleaved(hip, oracle):
    """the arrangement of scripts/two_streams.py at batch 8: one handle per stream, both reading resident buffers, rounds interleaved without
    waiting for each other; the handles swap buffers between rounds.  One handle on the bit-exact four-per-wavefront kernel, one on automatic
    dispatch (lqr_qtol, contract (T))"""
    n, dims, B = 40, D.IK, 8
    lods = [P.lse_batch(20290200 + 100 * i, B, n, dims) for i in range(2)]
    refs = [oracle.lse_run(lod, dims, n) for lod in lods]
    bufs = [Placed(lod, 16) for lod in lods]
    case = dict(name="two_streams", n=n, caps=dims, dims=np.tile(np.asarray(dims, np.uint32), (B, 1)))
    hs, streams = [], []
    for policy in (4, 0):
        s = hip.BatchedLexLSE(B, n, dims)
        s.set_kernel_policy(policy)
        st = torch.cuda.Stream()
        s.set_stream(st.cuda_stream)
        hs.append(s), streams.append(st)
    for rnd in range(4):
        for i, s in enumerate(hs):
            s.setProblemDevice(bufs[(i + rnd) % 2].ptr)
        for s in hs:
            s.factorize_solve(keep_factor=False)
        for i, s in enumerate(hs):
            assert s.last_kernel() == ("lqr_quad<3,12,shift 7>", "lqr_qtol<3,12,shift 7>")[i]
            check_values(s, case, refs[(i + rnd) % 2], "BT"[i], False)
    for buf in bufs:
        buf.assert_untouched()
    for s in hs:
        s.close()

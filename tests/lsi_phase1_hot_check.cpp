// The hot-start options of phase 1 (modify_x_guess_enabled, modify_type_active_enabled, modify_type_inactive_enabled, set_min_init_ctr_violation) as the
// device's setup kernel runs them (lexls_amd/csrc/lsi_phase1_setup.h: p1_hot_working_set, p1_initial_v) on the host, against host LexLSI objects after
// begin(): all 16 combinations x with / without x0 x with / without v0 x simple bounds first / general only x capacity rows / ragged rows — every list,
// type, stamp, x, v and A x, the first equality problem's row references where the layouts agree, and the activation order LexLSI rebuilds behind
// formInitialWorkingSet, with a removal of a hot-activated constraint under deactivate_first_wrong_sign.  Stand-alone: g++ -std=c++17 -I include -I lexls_amd/csrc.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <lexls/lsi_runner.h>
#include "lsi_phase1_setup.h"

using namespace LexLS;

namespace
{
    int failures = 0;
#define CHECK(cond, ...)                                  \
    do                                                    \
    {                                                     \
        if (!(cond))                                      \
        {                                                 \
            failures++;                                   \
            std::printf("FAILED %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
        }                                                 \
    } while (0)

    /// an equality solver that records the problem the driver posts and "solves" it with the x it was told (so that a step is zero); its removal
    /// search names every LB / UB row of level 0 when asked to (the set deactivate_first_wrong_sign picks the first-activated of)
    class ScriptedLSE
    {
    public:
        void resize(Index nVar_, Index nObj_, Index *maxObjDim)
        {
            nVar = nVar_, nObjL = nObj_, cap = 0;
            for (Index k = 0; k < nObjL; k++) cap += maxObjDim[k];
            dims.assign(nObjL, 0), first_row.assign(nObjL, 0);
            row_src.assign(cap, 0), row_ld.assign(cap, 0), ctr_type.assign(cap, 0);
            fixed_idx.assign(nVar, 0), fixed_val.assign(nVar, 0.0), fixed_type.assign(nVar, 0);
            x.resize(nVar);
            x.setZero();
        }
        void setParameters(const ParametersLexLSE &) {}
        void setRegularizationFactor(Index, RealScalar) {}
        void setObjDim(Index *d)
        {
            Index r = 0;
            for (Index k = 0; k < nObjL; k++) dims[k] = d[k], first_row[k] = r, r += d[k];
            nFixedInit = 0, formed++;
            std::fill(row_ld.begin(), row_ld.end(), 0u);
        }
        bool setCtrIndexed(Index row, size_t first_element, Index ld, unsigned use_ub)
        {
            row_src[row] = static_cast<uint32_t>(first_element);
            row_ld[row]  = static_cast<uint32_t>(ld) | (use_ub ? 0x80000000u : 0u);
            return true;
        }
        void setCtrStrided(Index, const RealScalar *, Index, RealScalar) { std::abort(); }
        void setFixedVariablesCount(Index nf) { nfixed = nf; }
        void fixVariable(Index var, RealScalar val, ConstraintActivationType type = CTR_ACTIVE_UB)
        {
            fixed_idx[nFixedInit] = var, fixed_val[nFixedInit] = val, fixed_type[nFixedInit] = static_cast<uint8_t>(type);
            nFixedInit++;
        }
        void setCtrType(Index obj, Index k, ConstraintActivationType type) { ctr_type[first_row[obj] + k] = static_cast<uint8_t>(type); }
        void factorize() {}
        void solve() {}
        bool ObjectiveSensitivity(Index, Index &, int &, RealScalar, RealScalar, RealScalar &) { return false; }
        void ObjectiveSensitivity(Index level, RealScalar, RealScalar, std::vector<ConstraintInfo> &out)
        {
            out.clear();
            if (!name_level0 || level != 0) return;
            for (Index i = 0; i < dims[0]; i++)
                if (ctr_type[first_row[0] + i] != static_cast<uint8_t>(CTR_ACTIVE_EQ)) out.push_back(ConstraintInfo(0, i));
        }
        const dVectorType &get_x() const { return x; }
        Index getTotalRank() const { return 0; }
        Index getDim(Index k) const { return dims[k]; }
        Index getFixedVariablesCount() const { return nfixed; }

        Index nVar = 0, nObjL = 0, cap = 0, nfixed = 0, nFixedInit = 0;
        int formed = 0;
        bool name_level0 = false;
        std::vector<uint32_t> dims, first_row, row_src, row_ld, fixed_idx;
        std::vector<uint8_t> ctr_type, fixed_type;
        std::vector<double> fixed_val;
        dVectorType x;
    };
    typedef internal::LexLSI_T<ScriptedLSE> HostLSI;

    /// deterministic numbers in (-1, 1)
    double rnd(uint32_t &s)
    {
        s = s * 1664525u + 1013904223u;
        return (static_cast<double>(s >> 8) / 8388608.0) - 1.0;
    }

    /// One instance twice: as the host object sees it (dims rows per objective, leading dimension dims) and as the device holds it (capacity rows per
    /// objective, leading dimension cap; rows from dims on are absent and hold NaN)
    struct Case
    {
        Index nVar;
        std::vector<Index> dims, cap;
        std::vector<int32_t> types;
        std::vector<double> data, cdata;
        std::vector<Index> var;
        std::vector<uint32_t> cvar;
        std::vector<uint8_t> guess, cguess; // per row: 0 .. 2
        std::vector<double> x0, v0, cv0;
        StepShape sh; // of the capacity layout
        std::vector<uint32_t> cnt;
        bool ragged;
    };

    Case make_case(Index nVar, std::vector<Index> dims, std::vector<Index> cap, bool simple_first, uint32_t seed)
    {
        Case c;
        c.nVar = nVar, c.dims = dims, c.cap = cap, c.ragged = dims != cap;
        const double nan = std::numeric_limits<double>::quiet_NaN();
        std::memset(&c.sh, 0, sizeof(c.sh));
        StepShape &sh = c.sh;
        sh.n = nVar, sh.nObj = static_cast<uint32_t>(dims.size()), sh.tol_feasibility = 1e-13;
        uint64_t o = 0;
        uint32_t f = 0;
        for (uint32_t k = 0; k < sh.nObj; k++)
        {
            const bool simple = simple_first && k == 0;
            c.types.push_back(simple ? 1 : 0);
            sh.dim[k] = cap[k], sh.simple[k] = simple, sh.first[k] = f, sh.off[k] = o;
            const Index m = dims[k], M = cap[k], cols = simple ? 2 : nVar + 2;
            c.cnt.push_back(m);
            std::vector<double> blk((size_t)m * cols);
            if (simple)
                for (Index r = 0; r < m; r++) c.var.push_back((r * 5 + 1) % nVar), blk[r] = -0.5 - 0.125 * r, blk[r + m] = 0.25 + 0.25 * r;
            else
                for (Index r = 0; r < m; r++)
                {
                    for (Index j = 0; j < nVar; j++) blk[r + (size_t)j * m] = rnd(seed);
                    const double mid = rnd(seed);
                    blk[r + (size_t)nVar * m] = mid - 0.375, blk[r + (size_t)(nVar + 1) * m] = mid + 0.375;
                }
            if (!simple && m > 2) blk[1 + (size_t)(nVar + 1) * m] = blk[1 + (size_t)nVar * m]; // an equality
            c.data.insert(c.data.end(), blk.begin(), blk.end());
            for (Index j = 0; j < cols; j++)
                for (Index r = 0; r < M; r++) c.cdata.push_back(r < m ? blk[r + (size_t)j * m] : nan);
            for (Index r = 0; r < M; r++)
            {
                const uint8_t g = static_cast<uint8_t>((rnd(seed) + 1.0) * 1.5); // 0 .. 2
                const double v  = 0.25 * rnd(seed);
                if (r < m) c.guess.push_back(g), c.v0.push_back(v);
                c.cguess.push_back(r < m ? g : 0), c.cv0.push_back(r < m ? v : nan);
            }
            o += (uint64_t)M * cols, f += M;
        }
        sh.total = f, sh.SD = sh.n + 2 * f, sh.per_data = o, sh.dim0 = c.types[0] == 1 ? cap[0] : 0;
        for (Index r = 0; r < (c.types[0] == 1 ? cap[0] : 0); r++) c.cvar.push_back(r < dims[0] ? c.var[r] : 0xffffffffu);
        for (Index j = 0; j < nVar; j++) c.x0.push_back(1.5 * rnd(seed));
        return c;
    }

    uint32_t branch_total[P1B_COUNT];

    template <bool RAGGED>
    void compare(const Case &c, uint32_t flags16, bool with_x0, bool with_v0, bool with_guess)
    {
        const StepShape &sh = c.sh;
        const uint32_t total = sh.total, nObj = sh.nObj, n = sh.n, off = sh.dim0 ? 1 : 0, nObjL = nObj - off;
        ParametersLexLSI par;
        par.modify_x_guess_enabled = flags16 & 1, par.modify_type_active_enabled = (flags16 >> 1) & 1, par.modify_type_inactive_enabled = (flags16 >> 2) & 1;
        par.set_min_init_ctr_violation = !((flags16 >> 3) & 1);
        par.tol_feasibility = sh.tol_feasibility;
        char tag[160];
        std::snprintf(tag, sizeof(tag), "n=%u simple=%u ragged=%d flags=%x x0=%d v0=%d guess=%d", n, off, (int)RAGGED, flags16, (int)with_x0, (int)with_v0, (int)with_guess);

        // ---- the host driver ----
        runner::LsiProblem p = {c.nVar, static_cast<Index>(nObj), c.dims.data(), c.types.data(), c.data.data(), c.var.empty() ? NULL : c.var.data(),
                                with_guess ? c.guess.data() : NULL, with_x0 ? c.x0.data() : NULL, (with_x0 && with_v0) ? c.v0.data() : NULL};
        HostLSI lsi;
        runner::setup(lsi, p, par);
        lsi.begin();
        std::vector<internal::Objective> obj = lsi.getObjectives();
        dVectorType hx = lsi.get_x();
        if (!with_x0) // phase 1 of the objectives comes behind the first solve (lexlsi.h:350-361): run it here, on the x the device would have taken from it
        {
            hx.resize(n);
            for (uint32_t j = 0; j < n; j++) hx(j) = c.x0[j];
            for (uint32_t k = 0; k < nObj; k++)
                obj[k].phase1(hx, false, par.modify_type_active_enabled, par.modify_type_inactive_enabled, par.modify_x_guess_enabled, par.set_min_init_ctr_violation, par.tol_feasibility);
        }

        // ---- the shared header, as the setup kernel (with x0) and the finish kernel (without) call it ----
        const uint32_t *cnt = RAGGED ? c.cnt.data() : NULL;
        const uint8_t *guess = with_guess ? c.cguess.data() : NULL;
        const uint32_t *var  = c.cvar.empty() ? NULL : c.cvar.data();
        std::vector<uint8_t> cls(total, 0), cs(total, 0xee), hotmark(total, 0xee);
        std::vector<uint16_t> act(total, 0xeeee), ina(total, 0xeeee), ipos(total, 0xeeee), na(STEP_MAX_OBJ, 0xeeee);
        std::vector<uint32_t> stamp(total, 0x0eeeeeeeu);
        uint32_t next_stamp = 0;
        for (uint32_t k = 0; k < nObj; k++)
            for (uint32_t r = 0; r < c.cnt[k]; r++) cls[sh.first[k] + r] = p1_row_class(sh, c.cdata.data(), k, r);
        p1_build_working_set<RAGGED>(sh, cls.data(), guess, cs.data(), act.data(), ina.data(), ipos.data(), na.data(), stamp.data(), &next_stamp, cnt);
        std::vector<double> x(c.x0), x_before(c.x0);
        const uint32_t word = p1_hot_word(par);
        const uint32_t hot  = (with_x0 && !with_v0) ? word : 0u; // (BatchCtx::enqueue_phase1_setup)
        uint32_t branch[P1B_COUNT] = {0};
        if (hot & (P1_HOT_MODIFY_X | P1_HOT_TYPE_ACTIVE | P1_HOT_TYPE_INACTIVE))
            p1_hot_working_set<RAGGED>(sh, c.cdata.data(), var, x.data(), hot, cs.data(), act.data(), ina.data(), ipos.data(), na.data(), stamp.data(), &next_stamp, hotmark.data(), cnt, branch);
        if (!(hot & P1_HOT_MODIFY_X)) CHECK(x == x_before, "%s: x rewritten without modify_x_guess_enabled", tag);
        const bool midpoint = with_x0 ? (hot & P1_HOT_V_MIDPOINT) != 0 : (word & P1_HOT_V_MIDPOINT) != 0; // (setup kernel / finish kernel)

        // ---- x, lists, types, A x, v ----
        for (uint32_t j = 0; j < n; j++) CHECK(x[j] == hx(j), "%s: x[%u] = %a, the host %a", tag, j, x[j], hx(j));
        for (uint32_t k = 0; k < nObj; k++)
        {
            const uint32_t f = sh.first[k], rows = c.cnt[k];
            CHECK(na[k] == obj[k].getActiveCtrCount(), "%s: objective %u has %u active constraints, the host %u", tag, k, na[k], obj[k].getActiveCtrCount());
            for (Index a = 0; a < obj[k].getActiveCtrCount() && a < na[k]; a++)
                CHECK(act[f + a] == obj[k].getActiveCtrIndex(a) && cs[f + act[f + a]] == static_cast<uint8_t>(obj[k].getActiveCtrType(a)), "%s: objective %u active[%u] = %u, the host %u", tag, k, a,
                      act[f + a], obj[k].getActiveCtrIndex(a));
            CHECK(rows - na[k] == obj[k].getInactiveCtrCount(), "%s: objective %u inactive count", tag, k);
            for (Index i = 0; i < obj[k].getInactiveCtrCount() && i < rows - na[k]; i++)
                CHECK(ina[f + i] == obj[k].getInactiveCtrIndex(i) && ipos[f + ina[f + i]] == i, "%s: objective %u inactive[%u] = %u, the host %u", tag, k, i, ina[f + i], obj[k].getInactiveCtrIndex(i));
            for (uint32_t r = 0; r < rows; r++)
            {
                CHECK(cs[f + r] == static_cast<uint8_t>(obj[k].getCtrType(r)), "%s: objective %u row %u has type %u, the host %u", tag, k, r, cs[f + r], (unsigned)obj[k].getCtrType(r));
                const double ax = p1_ax(sh, c.cdata.data(), var, x.data(), k, r);
                CHECK(ax == obj[k].get_Ax()(r), "%s: objective %u row %u: A x = %a, the host %a", tag, k, r, ax, obj[k].get_Ax()(r));
                const double v = (with_x0 && with_v0) ? c.cv0[f + r]
                                                      : p1_initial_v(cs[f + r], ax, p1_bound(sh, c.cdata.data(), k, r, 0), p1_bound(sh, c.cdata.data(), k, r, 1), midpoint, sh.tol_feasibility, branch);
                CHECK(v == obj[k].get_v()(r), "%s: objective %u row %u: v = %a, the host %a", tag, k, r, v, obj[k].get_v()(r));
            }
            for (uint32_t r = rows; r < sh.dim[k]; r++) CHECK(cs[f + r] == 0, "%s: absent row %u of objective %u is active", tag, r, k);
        }
        for (uint32_t i = 0; i < P1B_COUNT; i++) branch_total[i] += branch[i];
        if (!with_x0) return; // (the driver's own lists wait for the first solve)

        // ---- stamps = positions in the driver's activation-order list ----
        const std::vector<ConstraintInfo> &order = lsi.getActivationOrder();
        CHECK(next_stamp == order.size(), "%s: next stamp %u, the host's list holds %zu", tag, next_stamp, order.size());
        CHECK(order.size() == lsi.getActiveCtrCount(), "%s: the host's list holds %zu entries for %u active constraints", tag, order.size(), lsi.getActiveCtrCount());
        for (size_t q = 0; q < order.size(); q++)
        {
            const uint32_t g = sh.first[order[q].get_obj_index()] + order[q].get_ctr_index();
            CHECK(cs[g] != 0 && stamp[g] == q, "%s: stamp of (%d, %d) is %u, its place in the host's list %zu", tag, order[q].get_obj_index(), order[q].get_ctr_index(), stamp[g], q);
        }
        CHECK(lsi.getActivationsCount() == 0 && lsi.getDeactivationsCount() == 0 && lsi.getWorkingSetLog().empty(), "%s: phase 1 counted or logged a working-set change", tag);

        // ---- the first equality problem (row references: where the two layouts are one) ----
        const ScriptedLSE &rec = lsi.getLexLSE();
        uint32_t cap = 0;
        for (uint32_t k = off; k < nObj; k++) cap += sh.dim[k];
        std::vector<uint32_t> dims(nObjL, 0xeeeeeeeeu), nfixed(1, 0xeeeeeeeeu), fixed_idx(n, 0xeeeeeeeeu), row_src(cap, 0xeeeeeeeeu), row_ld(cap, 0xeeeeeeeeu);
        std::vector<double> fixed_val(n, -7.0), cdata(c.cdata);
        std::vector<uint8_t> fixed_type(n, 0xee), ctr_type(cap, 0xee);
        const EqualityProblemSlab slab = {dims.data(), nfixed.data(), fixed_idx.data(), fixed_val.data(), row_src.data(), row_ld.data(), fixed_type.data(), ctr_type.data()};
        lsi_form_equality_problem(sh, off, nObjL, cap, 0, cdata.data(), var, na.data(), act.data(), cs.data(), slab, 0, 1u);
        uint32_t rows = 0;
        for (uint32_t k = 0; k < nObjL; k++)
        {
            CHECK(dims[k] == rec.dims[k], "%s: level %u has %u rows, the host %u", tag, k, dims[k], rec.dims[k]);
            rows += rec.dims[k];
        }
        if (off)
        {
            CHECK(nfixed[0] == rec.nfixed, "%s: %u fixed variables, the host %u", tag, nfixed[0], rec.nfixed);
            for (uint32_t i = 0; i < rec.nfixed && i < nfixed[0]; i++)
                CHECK(fixed_idx[i] == rec.fixed_idx[i] && fixed_val[i] == rec.fixed_val[i] && fixed_type[i] == rec.fixed_type[i], "%s: fixed variable %u", tag, i);
        }
        for (uint32_t r = 0; r < rows && r < cap; r++)
        {
            CHECK(ctr_type[r] == rec.ctr_type[r] && (row_ld[r] >> 31) == (rec.row_ld[r] >> 31), "%s: row %u: type / bound", tag, r);
            if (!RAGGED) CHECK(row_src[r] == rec.row_src[r] && row_ld[r] == rec.row_ld[r], "%s: row %u: (%u, %08x), the host (%u, %08x)", tag, r, row_src[r], row_ld[r], rec.row_src[r], rec.row_ld[r]);
        }
    }

    /// A constraint formInitialWorkingSet activated leaves again under deactivate_first_wrong_sign: the walk over the activation order finds it (the
    /// reference's list does not hold it: the walk runs off the list and the erase takes end()), the one that entered first goes
    void remove_after_hot_activation(const Case &c, bool with_guess)
    {
        ParametersLexLSI par;
        par.modify_type_inactive_enabled = true, par.modify_type_active_enabled = true, par.deactivate_first_wrong_sign = true;
        runner::LsiProblem p = {c.nVar, static_cast<Index>(c.dims.size()), c.dims.data(), c.types.data(), c.data.data(), NULL, with_guess ? c.guess.data() : NULL, c.x0.data(), NULL};
        HostLSI lsi;
        lsi.getLexLSE().name_level0 = true;
        runner::setup(lsi, p, par);
        lsi.begin();
        for (Index j = 0; j < c.nVar; j++) lsi.getLexLSE().x(j) = c.x0[j]; // the "solution" is the guess: a zero step, nothing blocks
        const std::vector<ConstraintInfo> before = lsi.getActivationOrder();
        int hot_in_list = 0; // entries of objective 0 that are no equalities: the guess's and formInitialWorkingSet's
        ConstraintInfo expect;
        for (size_t q = before.size(); q-- > 0;)
            if (before[q].get_obj_index() == 0 && lsi.getObjectives()[0].getCtrType(before[q].get_ctr_index()) != CTR_ACTIVE_EQ) expect = before[q], hot_in_list++;
        CHECK(hot_in_list > 0, "remove-after-hot-activation: objective 0 has no LB / UB constraint");
        CHECK(before.size() == lsi.getActiveCtrCount(), "remove-after-hot-activation: %zu entries for %u active constraints", before.size(), lsi.getActiveCtrCount());
        lsi.advance(); // phase 1's solve, iteration 0: not blocked
        CHECK(lsi.need() == HostLSI::NEED_SENSITIVITY, "remove-after-hot-activation: iteration 0 was blocked");
        if (lsi.need() != HostLSI::NEED_SENSITIVITY) return;
        lsi.advance(); // the removal
        const std::vector<ConstraintInfo> &after = lsi.getActivationOrder();
        CHECK(lsi.getDeactivationsCount() == 1 && after.size() + 1 == before.size(), "remove-after-hot-activation: %u removals, list %zu -> %zu", lsi.getDeactivationsCount(), before.size(), after.size());
        CHECK(lsi.getObjectives()[0].getCtrType(expect.get_ctr_index()) == CTR_INACTIVE, "remove-after-hot-activation: (0, %d), first in the list, is still active", expect.get_ctr_index());
        CHECK(std::find(after.begin(), after.end(), expect) == after.end(), "remove-after-hot-activation: the removed constraint is still in the list");
    }
} // namespace

int main()
{
    std::vector<Case> cases;
    cases.push_back(make_case(6, {4, 3, 5, 4}, {4, 3, 5, 4}, true, 101u));
    cases.push_back(make_case(8, {3, 5, 4}, {3, 5, 4}, false, 202u));
    cases.push_back(make_case(6, {3, 2, 5, 3}, {4, 3, 5, 4}, true, 303u));
    cases.push_back(make_case(8, {3, 4, 2}, {3, 5, 4}, false, 404u));
    size_t runs = 0;
    for (const Case &c : cases)
        for (uint32_t flags = 0; flags < 16; flags++)
            for (int x0 = 0; x0 < 2; x0++)
                for (int v0 = 0; v0 < 2; v0++)
                    for (int guess = 0; guess < 2; guess++, runs++)
                        if (c.ragged)
                            compare<true>(c, flags, x0 != 0, v0 != 0, guess != 0);
                        else
                            compare<false>(c, flags, x0 != 0, v0 != 0, guess != 0);
    static const char *names[P1B_COUNT] = {"inactive->LB", "inactive->UB", "LB kept", "LB->inactive", "LB->UB", "UB kept", "UB->inactive", "UB->LB", "EQ untouched",
                                           "x: inactive->midpoint", "x: LB->lb", "x: UB/EQ->ub", "v: inside->0", "v: outside->midpoint residual"};
    for (uint32_t i = 0; i < P1B_COUNT; i++)
    {
        std::printf("branch %-30s %u\n", names[i], branch_total[i]);
        CHECK(branch_total[i] > 0, "branch '%s' was never taken", names[i]);
    }
    remove_after_hot_activation(cases[1], false);
    remove_after_hot_activation(cases[1], true);
    if (failures)
    {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("phase 1 hot start ok (%zu runs)\n", runs);
    return 0;
}

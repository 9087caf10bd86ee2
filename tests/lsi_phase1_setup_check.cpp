// The serial part of phase 1 on the device (lexls_amd/csrc/lsi_phase1_setup.h) on the host, against the host driver: for a handful of small
// hierarchies every list, type, stamp, count and row reference the shared header produces is compared with what a LexLSI_T instance holds after
// runner::setup + begin() (its working sets, its activation order, the equality problem it posts).  Stand-alone: g++ -std=c++17 -I include -I lexls_amd/csrc.
#include <cstdio>
#include <cstdlib>
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

    /// an equality solver that records the problem the driver posts (what SlotLSE writes into a group's in block) and solves nothing
    class RecordingLSE
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
        void ObjectiveSensitivity(Index, RealScalar, RealScalar, std::vector<ConstraintInfo> &) {}
        const dVectorType &get_x() const { return x; }
        Index getTotalRank() const { return 0; }
        Index getDim(Index k) const { return dims[k]; }
        Index getFixedVariablesCount() const { return nfixed; }

        Index nVar = 0, nObjL = 0, cap = 0, nfixed = 0, nFixedInit = 0;
        int formed = 0;
        std::vector<uint32_t> dims, first_row, row_src, row_ld, fixed_idx;
        std::vector<uint8_t> ctr_type, fixed_type;
        std::vector<double> fixed_val;
        dVectorType x;
    };
    typedef internal::LexLSI_T<RecordingLSE> HostLSI;

    struct Hierarchy
    {
        const char *name;
        Index nVar;
        std::vector<Index> dims;
        std::vector<int32_t> types;
        std::vector<double> data; // flat, per objective column-major
        std::vector<Index> var;
        std::vector<uint8_t> guess; // empty: none
        bool with_x0;
    };

    StepShape shape_of(const Hierarchy &h)
    {
        StepShape sh;
        std::memset(&sh, 0, sizeof(sh));
        uint64_t o = 0;
        uint32_t f = 0;
        sh.n = h.nVar, sh.nObj = static_cast<uint32_t>(h.dims.size());
        for (uint32_t k = 0; k < sh.nObj; k++)
        {
            sh.dim[k] = h.dims[k], sh.simple[k] = h.types[k] == 1, sh.first[k] = f, sh.off[k] = o;
            o += static_cast<uint64_t>(h.dims[k]) * (h.types[k] == 1 ? 2 : h.nVar + 2);
            f += h.dims[k];
        }
        sh.total = f, sh.SD = sh.n + 2 * f, sh.per_data = o, sh.dim0 = h.types[0] == 1 ? h.dims[0] : 0;
        return sh;
    }

    /// deterministic numbers in (-1, 1)
    double rnd(uint32_t &s)
    {
        s = s * 1664525u + 1013904223u;
        return (static_cast<double>(s >> 8) / 8388608.0) - 1.0;
    }

    /// a hierarchy with random rows and lb < ub everywhere; the callers plant the special rows
    Hierarchy random_hierarchy(const char *name, Index nVar, std::vector<Index> dims, bool simple_first, uint32_t seed)
    {
        Hierarchy h;
        h.name = name, h.nVar = nVar, h.dims = dims, h.with_x0 = false;
        for (size_t k = 0; k < dims.size(); k++)
        {
            const bool simple = simple_first && k == 0;
            h.types.push_back(simple ? 1 : 0);
            const Index m = dims[k];
            if (simple)
            {
                for (Index c = 0; c < m; c++) h.var.push_back((c * 3 + 1) % nVar);
                for (Index c = 0; c < m; c++) h.data.push_back(-1.0 - 0.125 * c);
                for (Index c = 0; c < m; c++) h.data.push_back(1.0 + 0.25 * c);
            }
            else
            {
                for (Index j = 0; j < nVar; j++)
                    for (Index c = 0; c < m; c++) h.data.push_back(rnd(seed));
                std::vector<double> mid(m);
                for (Index c = 0; c < m; c++) mid[c] = rnd(seed), h.data.push_back(mid[c] - 0.5);
                for (Index c = 0; c < m; c++) h.data.push_back(mid[c] + 0.5);
            }
        }
        return h;
    }
    double &lb_of(Hierarchy &h, const StepShape &sh, uint32_t k, uint32_t c) { return h.data[sh.off[k] + c + (sh.simple[k] ? 0 : (size_t)sh.n * sh.dim[k])]; }
    double &ub_of(Hierarchy &h, const StepShape &sh, uint32_t k, uint32_t c) { return h.data[sh.off[k] + c + (sh.simple[k] ? sh.dim[k] : (size_t)(sh.n + 1) * sh.dim[k])]; }
    void zero_normal(Hierarchy &h, const StepShape &sh, uint32_t k, uint32_t c)
    {
        for (uint32_t j = 0; j < sh.n; j++) h.data[sh.off[k] + c + (size_t)j * sh.dim[k]] = 0.0;
    }

    /// instance `slot` of a batch of `slots`: the shared header's output against the host driver's
    void compare(const Hierarchy &h, uint32_t slot, uint32_t slots)
    {
        const StepShape sh   = shape_of(h);
        const uint32_t total = sh.total, nObj = sh.nObj, off = sh.dim0 ? 1 : 0, nObjL = nObj - off, n = sh.n;
        uint32_t cap         = 0;
        for (uint32_t k = off; k < nObj; k++) cap += sh.dim[k];

        // ---- the host driver ----
        std::vector<double> x0(n, 0.125);
        runner::LsiProblem p = {h.nVar, static_cast<Index>(nObj), h.dims.data(), h.types.data(), h.data.data(), h.var.empty() ? NULL : h.var.data(),
                                h.guess.empty() ? NULL : h.guess.data(), h.with_x0 ? x0.data() : NULL};
        HostLSI lsi;
        runner::setup(lsi, p, ParametersLexLSI());
        lsi.begin();
        const RecordingLSE &rec = lsi.getLexLSE();
        CHECK(rec.formed == 1, "%s: the host driver formed %d equality problems in begin()", h.name, rec.formed);

        // ---- the shared header, as the setup kernel calls it ----
        std::vector<uint8_t> cls(total), cs(total, 0xee);
        std::vector<uint16_t> act(total, 0xeeee), ina(total, 0xeeee), ipos(total, 0xeeee), na(STEP_MAX_OBJ, 0xeeee);
        std::vector<uint32_t> stamp(total, 0xeeeeeeeeu);
        uint32_t next_stamp = 0xeeeeeeeeu;
        std::vector<double> data(h.data);
        std::vector<uint32_t> var(h.var.begin(), h.var.end());
        CHECK(p1_instance_fault(sh, data.data(), var.empty() ? NULL : var.data(), h.guess.empty() ? NULL : h.guess.data(), cls.data()) == P1_OK, "%s: a fault in a valid instance", h.name);
        p1_build_working_set(sh, cls.data(), h.guess.empty() ? NULL : h.guess.data(), cs.data(), act.data(), ina.data(), ipos.data(), na.data(), stamp.data(), &next_stamp);
        std::vector<uint32_t> dims((size_t)slots * (nObjL ? nObjL : 1), 0xeeeeeeeeu), nfixed(slots, 0xeeeeeeeeu), fixed_idx((size_t)slots * n, 0xeeeeeeeeu),
            row_src((size_t)slots * cap, 0xeeeeeeeeu), row_ld((size_t)slots * cap, 0xeeeeeeeeu);
        std::vector<double> fixed_val((size_t)slots * n, -7.0);
        std::vector<uint8_t> fixed_type((size_t)slots * n, 0xee), ctr_type((size_t)slots * cap, 0xee);
        const EqualityProblemSlab slab = {dims.data(), nfixed.data(), fixed_idx.data(), fixed_val.data(), row_src.data(), row_ld.data(), fixed_type.data(), ctr_type.data()};
        for (uint32_t lane = 0; lane < 3; lane++) // three "lanes" one after the other: the same problem as one
            lsi_form_equality_problem(sh, off, nObjL, cap, slot, data.data(), var.empty() ? NULL : var.data(), na.data(), act.data(), cs.data(), slab, lane, 3u);

        // ---- working sets: lists, types, counts (workingset.h order) ----
        const std::vector<internal::Objective> &obj = lsi.getObjectives();
        for (uint32_t k = 0; k < nObj; k++)
        {
            const uint32_t f = sh.first[k];
            CHECK(na[k] == obj[k].getActiveCtrCount(), "%s: objective %u has %u active constraints, the host %u", h.name, k, na[k], obj[k].getActiveCtrCount());
            for (Index a = 0; a < obj[k].getActiveCtrCount() && a < na[k]; a++)
            {
                CHECK(act[f + a] == obj[k].getActiveCtrIndex(a), "%s: objective %u active[%u] = %u, the host %u", h.name, k, a, act[f + a], obj[k].getActiveCtrIndex(a));
                CHECK(cs[f + act[f + a]] == static_cast<uint8_t>(obj[k].getActiveCtrType(a)), "%s: objective %u active[%u] has type %u", h.name, k, a, cs[f + act[f + a]]);
            }
            CHECK(sh.dim[k] - na[k] == obj[k].getInactiveCtrCount(), "%s: objective %u inactive count", h.name, k);
            for (Index i = 0; i < obj[k].getInactiveCtrCount(); i++)
            {
                CHECK(ina[f + i] == obj[k].getInactiveCtrIndex(i), "%s: objective %u inactive[%u] = %u, the host %u", h.name, k, i, ina[f + i], obj[k].getInactiveCtrIndex(i));
                CHECK(ipos[f + obj[k].getInactiveCtrIndex(i)] == i, "%s: objective %u position of inactive constraint %u", h.name, k, obj[k].getInactiveCtrIndex(i));
            }
            for (uint32_t c = 0; c < sh.dim[k]; c++)
                CHECK(cs[f + c] == static_cast<uint8_t>(obj[k].getCtrType(c)), "%s: objective %u constraint %u has type %u, the host %u", h.name, k, c, cs[f + c], (unsigned)obj[k].getCtrType(c));
        }
        for (uint32_t k = nObj; k < STEP_MAX_OBJ; k++) CHECK(na[k] == 0, "%s: na[%u] != 0", h.name, k);
        // ---- stamps = positions in the reference's WS list ----
        const std::vector<ConstraintInfo> &order = lsi.getActivationOrder();
        CHECK(next_stamp == order.size(), "%s: next stamp %u, the host's list holds %zu", h.name, next_stamp, order.size());
        for (size_t q = 0; q < order.size(); q++)
            CHECK(stamp[sh.first[order[q].get_obj_index()] + order[q].get_ctr_index()] == q, "%s: stamp of (%d, %d) is %u, its place in the host's list %zu", h.name,
                  order[q].get_obj_index(), order[q].get_ctr_index(), stamp[sh.first[order[q].get_obj_index()] + order[q].get_ctr_index()], q);
        // ---- the first equality problem ----
        for (uint32_t k = 0; k < nObjL; k++) CHECK(dims[(size_t)slot * nObjL + k] == rec.dims[k], "%s: level %u has %u rows, the host %u", h.name, k, dims[(size_t)slot * nObjL + k], rec.dims[k]);
        if (off)
        {
            CHECK(nfixed[slot] == rec.nfixed, "%s: %u fixed variables, the host %u", h.name, nfixed[slot], rec.nfixed);
            for (uint32_t i = 0; i < rec.nfixed; i++)
            {
                const size_t q = (size_t)slot * n + i;
                CHECK(fixed_idx[q] == rec.fixed_idx[i] && fixed_val[q] == rec.fixed_val[i] && fixed_type[q] == rec.fixed_type[i], "%s: fixed variable %u: (%u, %g, %u), the host (%u, %g, %u)", h.name,
                      i, fixed_idx[q], fixed_val[q], fixed_type[q], rec.fixed_idx[i], rec.fixed_val[i], rec.fixed_type[i]);
            }
        }
        uint32_t rows = 0;
        for (uint32_t k = 0; k < nObjL; k++) rows += rec.dims[k];
        for (uint32_t r = 0; r < cap; r++)
        {
            const size_t q = (size_t)slot * cap + r;
            CHECK(row_ld[q] == rec.row_ld[r], "%s: row %u: ld word %08x, the host %08x", h.name, r, row_ld[q], rec.row_ld[r]);
            if (r < rows) CHECK(row_src[q] == rec.row_src[r] && ctr_type[q] == rec.ctr_type[r], "%s: row %u: (%u, %u), the host (%u, %u)", h.name, r, row_src[q], ctr_type[q], rec.row_src[r], rec.ctr_type[r]);
        }
        // nothing outside the slot's slices was written
        for (uint32_t s = 0; s < slots; s++)
            if (s != slot)
            {
                CHECK(nfixed[s] == 0xeeeeeeeeu, "%s: nfixed of slot %u written", h.name, s);
                for (uint32_t r = 0; r < cap; r++) CHECK(row_ld[(size_t)s * cap + r] == 0xeeeeeeeeu && row_src[(size_t)s * cap + r] == 0xeeeeeeeeu, "%s: rows of slot %u written", h.name, s);
                for (uint32_t i = 0; i < n; i++) CHECK(fixed_idx[(size_t)s * n + i] == 0xeeeeeeeeu, "%s: fixed variables of slot %u written", h.name, s);
            }
    }

    void expect_fault(Hierarchy h, uint32_t code, const char *what)
    {
        const StepShape sh = shape_of(h);
        std::vector<uint8_t> cls(sh.total);
        std::vector<uint32_t> var(h.var.begin(), h.var.end());
        const uint32_t got = p1_instance_fault(sh, h.data.data(), var.empty() ? NULL : var.data(), h.guess.empty() ? NULL : h.guess.data(), cls.data());
        CHECK(got == code, "%s: fault %u expected, %u found", what, code, got);
        CHECK((p1_fault_text(code)[0] != 0) == (code != P1_OK), "%s: text of fault %u", what, code);
    }
} // namespace

int main()
{
    std::vector<Hierarchy> all;
    {
        Hierarchy h = random_hierarchy("general only", 6, {3, 4, 2}, false, 11u);
        all.push_back(h);
        h.name = "general only, x0", h.with_x0 = true;
        all.push_back(h);
    }
    {
        Hierarchy h    = random_hierarchy("simple bounds first", 7, {4, 3, 5}, true, 23u);
        all.push_back(h);
    }
    {
        Hierarchy h    = random_hierarchy("rows with lb == ub", 5, {3, 4, 3}, false, 37u);
        StepShape sh   = shape_of(h);
        ub_of(h, sh, 0, 1) = lb_of(h, sh, 0, 1);         // an equality in the first objective
        ub_of(h, sh, 1, 3) = lb_of(h, sh, 1, 3) + 5e-16; // within isEqual's 1e-15
        ub_of(h, sh, 1, 0) = lb_of(h, sh, 1, 0);
        zero_normal(h, sh, 1, 0);                        // lb == ub, zero normal: stays inactive
        for (uint32_t c = 0; c < 3; c++) ub_of(h, sh, 2, c) = lb_of(h, sh, 2, c); // a whole objective of equalities
        all.push_back(h);
        h.name  = "rows with lb == ub, guess";
        h.guess = {2, 1, 0, /**/ 1, 0, 2, 1, /**/ 3, 0, 1}; // names active rows (0,1), (1,3), (2,0), (2,2), the zero-normal row, an EQ flag
        all.push_back(h);
        h.name = "rows with lb == ub, guess, x0", h.with_x0 = true;
        all.push_back(h);
    }
    {
        Hierarchy h  = random_hierarchy("a simple bound with lb == ub", 8, {5, 4, 3}, true, 41u);
        StepShape sh = shape_of(h);
        ub_of(h, sh, 0, 2) = lb_of(h, sh, 0, 2) = 0.375;
        ub_of(h, sh, 2, 1) = lb_of(h, sh, 2, 1);
        all.push_back(h);
        h.name  = "a simple bound with lb == ub, guess";
        h.guess = {1, 0, 2, 3, 2, /**/ 0, 2, 0, 1, /**/ 1, 1, 0}; // (0,2) and (2,1) are active already; (0,3) is an EQ flag
        all.push_back(h);
        h.name  = "a guess that activates everything";
        h.guess = {1, 2, 1, 2, 1, /**/ 2, 1, 2, 1, /**/ 1, 2, 1};
        all.push_back(h);
    }
    for (const Hierarchy &h : all)
    {
        compare(h, 0, 1);
        compare(h, 1, 3);
    }
    // ---- the four input checks ----
    {
        Hierarchy ok = random_hierarchy("faults", 8, {5, 4, 3}, true, 53u);
        StepShape sh = shape_of(ok);
        expect_fault(ok, P1_OK, "a valid instance");
        Hierarchy h = ok;
        lb_of(h, sh, 1, 2) = ub_of(h, sh, 1, 2) + 1.0;
        expect_fault(h, P1_LB_ABOVE_UB, "lb > ub in a general row");
        h = ok;
        lb_of(h, sh, 0, 4) = ub_of(h, sh, 0, 4) + 1e-3;
        expect_fault(h, P1_LB_ABOVE_UB, "lb > ub in a simple bound");
        h = ok;
        lb_of(h, sh, 1, 2) = ub_of(h, sh, 1, 2) + 5e-16; // (the reference tests isEqual first: no fault)
        expect_fault(h, P1_OK, "lb above ub within isEqual's tolerance");
        h = ok;
        h.var[3] = h.var[0];
        expect_fault(h, P1_VAR_DUPLICATE, "duplicate variable indices");
        h = ok;
        h.var[4] = 8;
        expect_fault(h, P1_VAR_RANGE, "a variable index >= nVar");
        h = ok;
        h.guess.assign(sh.total, 0);
        h.guess[7] = 4;
        expect_fault(h, P1_GUESS_TYPE, "a guess flag above 3");
        h.guess[7] = 3;
        expect_fault(h, P1_OK, "a guess flag of 3");
        // the host driver agrees on the two faults it knows
        for (int which = 0; which < 2; which++)
        {
            h = ok;
            if (which == 0)
                lb_of(h, sh, 1, 2) = ub_of(h, sh, 1, 2) + 1.0;
            else
                h.var[3] = h.var[0];
            bool thrown = false;
            try
            {
                runner::LsiProblem p = {h.nVar, 3, h.dims.data(), h.types.data(), h.data.data(), h.var.data(), NULL, NULL};
                HostLSI lsi;
                runner::setup(lsi, p, ParametersLexLSI());
            }
            catch (const Exception &)
            {
                thrown = true;
            }
            CHECK(thrown, "the host driver accepts fault %d", which);
        }
    }
    if (failures)
    {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("phase 1 setup ok (%zu hierarchies)\n", all.size());
    return 0;
}

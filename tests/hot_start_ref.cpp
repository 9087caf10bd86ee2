// Expected values for tests/test_gpu_lsi_hot_start.py: the host LexLSI driver over the CPU equality solver of oracle/lexlse_oracle.h, one instance at a
// time, with the 17 parameters of the C ABI.  Reads a batch from stdin (numbers as text, doubles as hex floats) and prints per instance x, info6,
// active, v as hex doubles, the working-set log, the branches phase 1 took (counted with lsi_phase1_setup.h on the same instance) and how many of
// the constraints phase 1 activated left the working set again later.  Optional inputs: regularization factors (one per objective), per-instance
// objective row counts (the instance is then ONE LexLSI of the shortened dims, its rows taken from the capacity layout and its results written back
// into it, absent rows zero) and a request for LexLSI::getLambda (nObj x total, the layout of lexls_lsi_batch_run_device_ex's d_lambda).  Stand-alone: g++ -std=c++17 -ffp-contract=off -I include -I oracle -I lexls_amd/csrc.
#include "lexlse_oracle.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <lexls/lsi_runner.h>
#include "lsi_phase1_setup.h"

using namespace LexLS;
typedef internal::LexLSI_T<lexls_oracle::LexLSE> OLSI;

static double rd()
{
    double v = 0;
    if (std::scanf("%la", &v) != 1) std::exit(3);
    return v;
}
static unsigned ru()
{
    unsigned v = 0;
    if (std::scanf("%u", &v) != 1) std::exit(3);
    return v;
}

int main()
{
    const unsigned nVar = ru(), nObj = ru(), batch = ru(), has_guess = ru(), has_x0 = ru(), has_counts = ru(), has_reg = ru(), want_lambda = ru();
    std::vector<Index> dims(nObj);
    std::vector<int32_t> types(nObj);
    for (auto &d : dims) d = ru();
    for (auto &t : types) t = (int32_t)ru();
    double prm[17];
    for (double &p : prm) p = rd();
    std::vector<double> reg(nObj, 0.0);
    if (has_reg)
        for (double &f : reg) f = rd();
    ParametersLexLSI par;
    par.max_number_of_factorizations = (Index)prm[0], par.tol_linear_dependence = prm[1], par.tol_wrong_sign_lambda = prm[2], par.tol_correct_sign_lambda = prm[3];
    par.tol_feasibility = prm[4], par.cycling_handling_enabled = prm[5] != 0, par.cycling_max_counter = (Index)prm[6], par.cycling_relax_step = prm[7];
    par.deactivate_first_wrong_sign = prm[8] != 0, par.regularization_type = (RegularizationType)(int)prm[9], par.variable_regularization_factor = prm[10];
    par.max_number_of_CG_iterations = (Index)prm[11];
    par.modify_x_guess_enabled = prm[12] != 0, par.modify_type_active_enabled = prm[13] != 0, par.modify_type_inactive_enabled = prm[14] != 0;
    par.set_min_init_ctr_violation = prm[15] != 0, par.use_phase1_v0 = prm[16] != 0;
    par.log_working_set_enabled = true;

    StepShape sh;
    std::memset(&sh, 0, sizeof(sh));
    sh.n = nVar, sh.nObj = nObj, sh.tol_feasibility = par.tol_feasibility;
    for (unsigned k = 0; k < nObj; k++)
    {
        sh.dim[k] = dims[k], sh.simple[k] = types[k] == 1, sh.first[k] = sh.total, sh.off[k] = sh.per_data;
        sh.per_data += (uint64_t)dims[k] * (types[k] == 1 ? 2 : nVar + 2), sh.total += dims[k];
    }
    sh.dim0 = types[0] == 1 ? dims[0] : 0, sh.SD = nVar + 2 * sh.total;
    const unsigned total = sh.total;
    uint32_t branch[P1B_COUNT] = {0};
    unsigned removed_hot = 0;
    for (unsigned b = 0; b < batch; b++)
    {
        std::vector<double> data(sh.per_data), x0(nVar), x(nVar), v(total);
        std::vector<Index> var(sh.dim0);
        std::vector<uint32_t> var32(sh.dim0);
        std::vector<uint8_t> guess(total), active(total);
        std::vector<Index> cnt(dims);
        if (has_counts)
            for (auto &c : cnt) c = ru();
        for (double &d : data) d = rd();
        for (unsigned c = 0; c < sh.dim0; c++) var32[c] = var[c] = ru();
        if (has_guess)
            for (auto &g : guess) g = (uint8_t)ru();
        if (has_x0)
            for (double &d : x0) d = rd();
        // the instance as one LexLSI object sees it: the first cnt[k] rows of every objective, leading dimension cnt[k]
        std::vector<double> sdata, sv;
        std::vector<uint8_t> sguess, sactive;
        unsigned stotal = 0;
        for (unsigned k = 0; k < nObj; k++)
        {
            const unsigned cols = types[k] == 1 ? 2 : nVar + 2;
            for (unsigned j = 0; j < cols; j++)
                for (unsigned r = 0; r < cnt[k]; r++) sdata.push_back(data[sh.off[k] + r + (size_t)j * dims[k]]);
            for (unsigned r = 0; r < cnt[k]; r++) sguess.push_back(guess[sh.first[k] + r]);
            stotal += cnt[k];
        }
        sv.assign(stotal, 0.0), sactive.assign(stotal, 0);
        runner::LsiProblem p = {nVar, nObj, cnt.data(), types.data(), sdata.data(), sh.dim0 ? var.data() : NULL, has_guess ? sguess.data() : NULL, has_x0 ? x0.data() : NULL, NULL,
                                has_reg ? reg.data() : NULL};
        OLSI lsi;
        runner::setup(lsi, p, par);
        lsi.solve();
        runner::LsiInfo info;
        runner::collect(lsi, p, x.data(), &info, sactive.data(), sv.data());
        std::fill(active.begin(), active.end(), 0), std::fill(v.begin(), v.end(), 0.0);
        for (unsigned k = 0, s = 0; k < nObj; s += cnt[k], k++)
            for (unsigned r = 0; r < cnt[k]; r++) active[sh.first[k] + r] = sactive[s + r], v[sh.first[k] + r] = sv[s + r];
        int32_t info6[6];
        std::memcpy(info6, &info, sizeof(info6));
        std::printf("x");
        for (double d : x) std::printf(" %a", d);
        std::printf("\ninfo");
        for (int32_t i : info6) std::printf(" %d", i);
        std::printf("\nactive");
        for (uint8_t a : active) std::printf(" %u", a);
        std::printf("\nv");
        for (double d : v) std::printf(" %a", d);
        const std::vector<WorkingSetLogEntry> &log = lsi.getWorkingSetLog();
        std::printf("\nlog %zu", log.size());
        for (const WorkingSetLogEntry &e : log) std::printf(" %d %d %d %d %d %a", (int)e.obj_index, (int)e.ctr_index, (int)e.ctr_type, e.cycling_detected ? 1 : 0, (int)e.rank, (double)e.alpha_or_lambda);
        std::printf("\n");
        if (want_lambda)
        {
            std::vector<dMatrixType> lam;
            lsi.getLambda(lam);
            std::printf("lambda");
            for (unsigned j = 0; j < nObj; j++)
                for (unsigned k = 0; k < nObj; k++)
                    for (unsigned r = 0; r < dims[k]; r++) std::printf(" %a", r < cnt[k] ? (double)lam[k](r, j) : 0.0);
            std::printf("\n");
        }
        // the branches of phase 1, counted on the same instance with the functions the device runs
        if (has_x0 && !has_counts)
        {
            std::vector<uint8_t> cls(total), cs(total), hotmark(total, 0);
            std::vector<uint16_t> act(total), ina(total), ipos(total), na(STEP_MAX_OBJ);
            std::vector<uint32_t> stamp(total, 0);
            uint32_t next = 0;
            p1_instance_fault(sh, data.data(), var32.data(), has_guess ? guess.data() : NULL, cls.data());
            p1_build_working_set(sh, cls.data(), has_guess ? guess.data() : NULL, cs.data(), act.data(), ina.data(), ipos.data(), na.data(), stamp.data(), &next);
            std::vector<double> xs(x0);
            const uint32_t hot = p1_hot_word(par);
            p1_hot_working_set(sh, data.data(), var32.data(), xs.data(), hot, cs.data(), act.data(), ina.data(), ipos.data(), na.data(), stamp.data(), &next, hotmark.data(), NULL, branch);
            for (unsigned k = 0; k < nObj; k++)
                for (unsigned c = 0; c < sh.dim[k]; c++)
                    p1_initial_v(cs[sh.first[k] + c], p1_ax(sh, data.data(), var32.data(), xs.data(), k, c), p1_bound(sh, data.data(), k, c, 0), p1_bound(sh, data.data(), k, c, 1),
                                 (hot & P1_HOT_V_MIDPOINT) != 0, sh.tol_feasibility, branch);
            std::vector<uint8_t> gone(total, 0);
            for (const WorkingSetLogEntry &e : log)
            {
                const unsigned g = sh.first[e.obj_index] + e.ctr_index;
                if (e.ctr_type == CTR_INACTIVE && hotmark[g] && !gone[g]) removed_hot++, gone[g] = 1;
                if (e.ctr_type != CTR_INACTIVE) gone[g] = 1; // (activated again by the iterations: no longer phase 1's)
            }
        }
    }
    std::printf("branches");
    for (uint32_t c : branch) std::printf(" %u", c);
    std::printf("\nremoved_hot %u\n", removed_hot);
    return 0;
}

// FOUR PROBLEMS PER WAVEFRONT, x-only, TOLERANCE-CONTRACT lexicographic-QR kernel for IK-sized batches — the bench kernel since round 3
// (lexlse.h:117-506 factorize() + :1015-1045 solve()).
//
// Contract (BASELINE north_star): column permutation, ranks and first columns EXACTLY those of the reference algorithm (first-maximum
// column pivoting on down-dated norms, rank test on the fresh squared norm against tol_linear_dependence), x within 1e-10.  Unlike
// lqr_quad_impl.h (same wavefront mapping, bit-identical to oracle/lexlse_oracle.h, still behind lexls_lse_set_kernel_policy(h, 4)) the
// VALUES are not held to the oracle's summation order, which buys:
//   * the reflector in RAW form.  With w = [c0 - beta; column tail] (= (c0 - beta) [1; essential part], lexlse.h:239-248) and
//     q = 1 / ((c0 - beta) beta):   H a = a + q (w.a) w.   The dot products w.a run on the raw pivot column BESIDE the sqrt / reciprocal
//     chain instead of behind it, and no essential part / tau is ever formed or broadcast (22 row broadcasts per pivot gone);
//   * NORMALISED images: a finished pivot row is kept as [R T | rhs] / R_jj.  The Gauss elimination of a later level's rows
//     (lexlse.h:431-471) then needs no multiplier product (a[r][P] -= a[r][c'] U'[c'][P]) and the back-substitution (lexlse.h:1015-1045) no
//     division.  The sign of beta cancels in U', so identity reflectors (tail == 0, last row of a level) need no special case;
//   * the search for pivot j+1 (butterflies on the down-dated norms, lexlse.h:205-206, :262-266) is issued right after row j of the block is
//     final, in front of the rank-one update of the rows below — latency chain and fma stream overlap;
//   * coalesced level loads: a level's rows arrive as 48-byte pieces of columns in consecutive lanes (a third of the line look-ups of the
//     column-per-lane load), are requested ONE LEVEL AHEAD (spread over the pivot steps of the level in front) and turned into the
//     position layout through a 2-KB LDS staging block per problem, half the rows at a time;
//   * triangular images (the part of [R_q T_q] below the diagonal is never read): 6,880 instead of 8,512 bytes per IK problem — what
//     makes room for the staging block at one wavefront per SIMD (4 x 10 KB per wavefront, 160 KB per CU).
// Mapping, position layout, index words: as in lqr_quad_impl.h (one problem per 16-lane DPP row, slot s of lane l = position 16 s + l - SIG
// when the level started, finished pivots in static lanes, row broadcasts with v_mov_b64_dpp row_newbcast).
//
// Shapes: every level of every problem has exactly MD rows (checked by the host: LseArgs::uniform_dim), no fixed variables, no
// regularization, n + 1 + SIG <= 16 NS, cap even, 16-byte aligned input.  Anything else takes the bit-exact kernels.
#pragma once
#include "lqr_quad_impl.h"

#include <cstdlib>


namespace lexls
{
    namespace
    {
        /// 1 / x to full double precision for normal x (v_rcp_f64 + two Newton steps); no scaling: |x| in [1e-290, 1e290]
        __device__ __forceinline__ double qt_rcp(double x)
        {
            double y = __builtin_amdgcn_rcp(x);
            double e = dfma(-x, y, 1.0);
            y        = dfma(y, e, y);
            e        = dfma(-x, y, 1.0);
            return dfma(y, e, y);
        }

        /// 1 / x to ~2^-50 (v_rcp_f64 + one Newton step): the factor of a rank-one update, whose own rounding is of that size
        __device__ __forceinline__ double qt_rcp1(double x)
        {
            const double y = __builtin_amdgcn_rcp(x);
            return dfma(y, dfma(-x, y, 1.0), y);
        }

        /// sqrt(x) for normal x (v_rsq_f64, one coupled iteration, two correction steps — the unscaled core of the library routine)
        __device__ __forceinline__ double qt_sqrt(double x)
        {
            const double y = __builtin_amdgcn_rsq(x);
            double g       = x * y;
            double h       = 0.5 * y;
            const double r = dfma(-h, g, 0.5);
            g              = dfma(g, r, g);
            h              = dfma(h, r, h);
            double d       = dfma(-g, g, x);
            g              = dfma(d, h, g);
            d              = dfma(-g, g, x);
            return dfma(d, h, g);
        }

        /// a double whose high word is `hi` and whose low word is that of v (sentinel norms: any low word gives a huge negative number)
        __device__ __forceinline__ double qt_with_hi(double v, int hi) { return __hiloint2double(hi, __double2loint(v)); }

#ifdef LEXLS_WAVE_STAMPS_FINE // = the S0 whose pivot steps are stamped (0: level 0 of the IK shape, 2: its last level)
#define FSTAMP(i) if constexpr (S0 == LEXLS_WAVE_STAMPS_FINE) STAMP(i)
#else
#define FSTAMP(i)
#endif
// Chain stamps (-DLEXLS_QTOL_CHAIN=<S0>): s_memtime behind an instruction that depends on the named value — the time at which that value is
// READY, without draining anything (the plain stamps wait for lgkmcnt(0) and disturb the chain they measure).  Seven points per pivot step.
#ifdef LEXLS_QTOL_CHAIN
#define CSTAMP(i, val)                                                                                     \
    if constexpr (S0 == LEXLS_QTOL_CHAIN)                                                                  \
    {                                                                                                      \
        int dummy_;                                                                                        \
        asm volatile("v_mov_b32 %1, %2\n\ts_memtime %0" : "=s"(ct[i]), "=v"(dummy_) : "v"(val));         \
    }
#define CSTAMP_COLLECT                                                                                     \
    if constexpr (S0 == LEXLS_QTOL_CHAIN)                                                                  \
    {                                                                                                      \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                 \
        if (cvalid)                                                                                        \
        {                                                                                                  \
            cacc[2] += ct[2] - cp1; cacc[3] += ct[3] - ct[2]; cacc[4] += ct[4] - ct[3];                     \
            cacc[5] += ct[5] - ct[4]; cacc[6] += ct[6] - ct[5]; cacc[0] += ct[0] - ct[6];                   \
        }                                                                                                  \
        cacc[1] += ct[1] - ct[0];                                                                          \
        cp1    = ct[1];                                                                                    \
        cvalid = true;                                                                                     \
    }
#else
#define CSTAMP(i, val)
#define CSTAMP_COLLECT
#endif
// per-level phase stamps of the diagnostic build: lambda[11 + 4 k + {0 load, 1 eliminate, 2 Householder, 3 level end}]
#ifdef LEXLS_WAVE_STAMPS
#define LSTAMP(ph)                                                                                   \
    {                                                                                                \
        const unsigned long long t_ = clock64();                                                     \
        if (gl == 0 && live) a.lambda[(size_t)b * (n + cap) + 11 + 4 * k + (ph)] = (double)(t_ - lst_t0); \
        lst_t0 = t_;                                                                                 \
    }
// ... and the elimination of a level split by step form: lambda[40 + 4 k + f], f = 0: the level head's requests for the first image rows, until
// they have arrived; f = 1, 2, 3: the steps with that many live slots.  One stamp where the form changes and one behind the last step, none
// between the steps of a form: a stamp waits for lgkmcnt(0), which would drain the rows in flight in every step.  The stamp that ends a form
// does drain them once, at that form's cost.
#define ESTAMP_DECL                                                \
    static_assert(NS <= 3, "four stamp places per level");         \
    unsigned long long est_acc[4] = {0, 0, 0, 0}, est_t0 = clock64();
#define ESTAMP(f)                                  \
    {                                              \
        const unsigned long long t_ = clock64();   \
        est_acc[f] += t_ - est_t0;                 \
        est_t0 = t_;                               \
    }
#define ESTAMP_END(fcmax)                                                                                               \
    {                                                                                                                   \
        const unsigned long long t_ = clock64();                                                                        \
        const int f_               = (fcmax) > 0 ? NS - ((fcmax) - 1 + SIG) / 16 : 0;                                   \
        _Pragma("unroll") for (int i_ = 0; i_ < 4; i_++)                                                                \
            if (gl == 0 && live) a.lambda[(size_t)b * (n + cap) + 40 + 4 * k + i_] = (double)(est_acc[i_] + (i_ == f_ ? t_ - est_t0 : 0ull)); \
    }
#else
#define LSTAMP(ph)
#define ESTAMP_DECL
#define ESTAMP(f)
#define ESTAMP_END(fcmax)
#endif
// Region marks (-DLEXLS_QTOL_MARKS, assembly only): a comment line "; qtol-region <name> [i [j]]" at the head of every phase and of every unrolled
// step, by which scripts/qtol_insn_table.py splits the kernel's assembly and weighs each part with its trip count.  The product build has none.
#ifdef LEXLS_QTOL_MARKS
#define QT_MARK(name) asm volatile("; qtol-region " name);
#define QT_MARK1(name, i) asm volatile("; qtol-region " name " %0" ::"i"(i));
#define QT_MARK2(name, i, j) asm volatile("; qtol-region " name " %0 %1" ::"n"(i), "n"(j));
#else
#define QT_MARK(name)
#define QT_MARK1(name, i)
#define QT_MARK2(name, i, j)
#endif
// ... of a phase that exists twice, in the peeled level 0 (constexpr bool L0 in scope: "level0-<name>") and in the level loop ("<name>")
#define QT_LMARK(name)        if constexpr (L0) { QT_MARK("level0-" name) } else { QT_MARK(name) }
#define QT_LMARK1(name, i)    if constexpr (L0) { QT_MARK1("level0-" name, i) } else { QT_MARK1(name, i) }
#define QT_LMARK2(name, i, j) if constexpr (L0) { QT_MARK2("level0-" name, i, j) } else { QT_MARK2(name, i, j) }
        /// f(integral_constant<int, I>) for I = B, B+1, ... while pred(I) holds: the first failing test leaves the whole remainder behind one branch
        template <int B, int E, class P, class F>
        __device__ __forceinline__ void qt_for_each_while(P &&pred, F &&f)
        {
            if constexpr (B < E)
            {
                if (pred(std::integral_constant<int, B>{}))
                {
                    f(std::integral_constant<int, B>{});
                    qt_for_each_while<B + 1, E>(pred, f);
                }
            }
        }

        typedef double qt_d2 __attribute__((ext_vector_type(2))); // 16 bytes as a native vector (the level pieces stay in registers)
        typedef qt_d2 qt_d2u __attribute__((aligned(8)));         // ... read at the alignment of a double (ragged levels)


        // ---- the level-ahead pieces live in FIXED accumulation registers a[184:255], managed by inline assembly -----------------------
        // A piece register that the compiler allocates must have ONE load site (two sites meet in register copies that wait for the loads in
        // flight: s_waitcnt vmcnt(0) in the middle of the pivot loop), but the requests have to be spread over the whole level in front —
        // Householder phase included, which exists in one instantiation per number of live slots — because the memory system takes what
        // every wave of the chip asks for at once at HBM speed only (scripts/ubench/loadpat.hip: ~8-10 k cycles per level and wave when
        // nothing else is done meanwhile).  So the compiler never sees these registers: piece t is a[184 + 4 t : 187 + 4 t], loaded and
        // stored by the statements below; the build checks that no other instruction of the code object names a184 .. a255
        // (scripts/check_qtol_regs.py, run by the Makefile).
#define QT_PF_LIST(X) X(0, 184, 187) X(1, 188, 191) X(2, 192, 195) X(3, 196, 199) X(4, 200, 203) X(5, 204, 207) X(6, 208, 211) X(7, 212, 215) X(8, 216, 219) \
    X(9, 220, 223) X(10, 224, 227) X(11, 228, 231) X(12, 232, 235) X(13, 236, 239) X(14, 240, 243) X(15, 244, 247) X(16, 248, 251) X(17, 252, 255)
        /// piece T <- 16 bytes at base (wave-uniform, in scalar registers) + byte offset (per lane): no vector address arithmetic per request
        template <int T>
        __device__ __forceinline__ void qt_pf_load(const double *base, uint32_t byte_offset)
        {
#define QT_PF_LOAD(t, lo, hi) \
    if constexpr (T == t) asm volatile("global_load_dwordx4 a[" #lo ":" #hi "], %0, %1" ::"v"(byte_offset), "s"(base) : "memory", "a" #lo, "a" #hi);
            QT_PF_LIST(QT_PF_LOAD)
#undef QT_PF_LOAD
        }
        template <int T>
        __device__ __forceinline__ void qt_pf_store_lds(int lds_byte_address)
        {
#define QT_PF_STORE(t, lo, hi) \
    if constexpr (T == t) asm volatile("ds_write_b128 %0, a[" #lo ":" #hi "]" ::"v"(lds_byte_address) : "memory");
            QT_PF_LIST(QT_PF_STORE)
#undef QT_PF_STORE
        }

        // ---- Gauss step with the row broadcast folded into the fma: d[r] = fma(bcast_L(s[r]), -u, d[r]), r = 0 .. MD-1, as v_fmac_f64_dpp
        // row_newbcast:L — one instruction per row instead of v_mov_b64_dpp + v_fma_f64 (scripts/ubench/fmac_dpp.hip: 5.7 against 4.4 + 4.4
        // cycles).  fma(l, -u, a) rounds as fma(-l, u, a).  A DPP read wants two wait states behind a VALU write of its source; the compiler
        // does not look inside inline assembly, so each block opens with s_nop 1 (what the compiler put in front may have written a source,
        // e.g. a reload from an accumulation register) and no row of a block reads what the row in front of it wrote.
        // Precondition: FULL EXEC.  gbc<> (update_dpp with bound_ctrl and old = 0) hands a zero to a row whose source lane is disabled; these
        // instructions carry no bound_ctrl, so a disabled source lane would suppress the write instead.  lqr_qtol's body is straight-line with
        // selects (rows beyond the batch run on a valid problem), every lane is enabled wherever the helpers are called.
#define QT_FD(i) "v_fmac_f64_dpp %[d" #i "], %[s" #i "], -%[u] row_newbcast:%[l] row_mask:0xf bank_mask:0xf\n\t"
#define QT_FS(i) "v_fmac_f64_dpp %[d" #i "], %[d" #i "], -%[u] row_newbcast:%[l] row_mask:0xf bank_mask:0xf\n\t"
#define QT_FO(i) [d##i] "+v"(d[i])
#define QT_FI(i) [s##i] "v"(s[i])
        /// another slot's rows: d (slot behind the pivot's) -= bcast_L(s) u, s = the rows of the pivot's slot
        template <int L, int MD>
        __device__ __forceinline__ void qt_gauss_dpp(double (&d)[MD], const double (&s)[MD], double u)
        {
            static_assert(MD == 8 || MD == 12, "operand lists below");
            if constexpr (MD == 8)
                asm volatile("s_nop 1\n\t" QT_FD(0) QT_FD(1) QT_FD(2) QT_FD(3) QT_FD(4) QT_FD(5) QT_FD(6) QT_FD(7)
                             : QT_FO(0), QT_FO(1), QT_FO(2), QT_FO(3), QT_FO(4), QT_FO(5), QT_FO(6), QT_FO(7)
                             : QT_FI(0), QT_FI(1), QT_FI(2), QT_FI(3), QT_FI(4), QT_FI(5), QT_FI(6), QT_FI(7), [u] "v"(u), [l] "n"(L));
            else
                asm volatile("s_nop 1\n\t" QT_FD(0) QT_FD(1) QT_FD(2) QT_FD(3) QT_FD(4) QT_FD(5) QT_FD(6) QT_FD(7) QT_FD(8) QT_FD(9) QT_FD(10) QT_FD(11)
                             : QT_FO(0), QT_FO(1), QT_FO(2), QT_FO(3), QT_FO(4), QT_FO(5), QT_FO(6), QT_FO(7), QT_FO(8), QT_FO(9), QT_FO(10), QT_FO(11)
                             : QT_FI(0), QT_FI(1), QT_FI(2), QT_FI(3), QT_FI(4), QT_FI(5), QT_FI(6), QT_FI(7), QT_FI(8), QT_FI(9), QT_FI(10), QT_FI(11),
                               [u] "v"(u), [l] "n"(L));
        }
        /// the pivot's own slot, LAST in its step (lane L of it becomes zero: U'[c'][c'] is 1): every row reads lane L of itself
        template <int L, int MD>
        __device__ __forceinline__ void qt_gauss_dpp_self(double (&d)[MD], double u)
        {
            static_assert(MD == 8 || MD == 12, "operand lists below");
            if constexpr (MD == 8)
                asm volatile("s_nop 1\n\t" QT_FS(0) QT_FS(1) QT_FS(2) QT_FS(3) QT_FS(4) QT_FS(5) QT_FS(6) QT_FS(7)
                             : QT_FO(0), QT_FO(1), QT_FO(2), QT_FO(3), QT_FO(4), QT_FO(5), QT_FO(6), QT_FO(7)
                             : [u] "v"(u), [l] "n"(L));
            else
                asm volatile("s_nop 1\n\t" QT_FS(0) QT_FS(1) QT_FS(2) QT_FS(3) QT_FS(4) QT_FS(5) QT_FS(6) QT_FS(7) QT_FS(8) QT_FS(9) QT_FS(10) QT_FS(11)
                             : QT_FO(0), QT_FO(1), QT_FO(2), QT_FO(3), QT_FO(4), QT_FO(5), QT_FO(6), QT_FO(7), QT_FO(8), QT_FO(9), QT_FO(10), QT_FO(11)
                             : [u] "v"(u), [l] "n"(L));
        }
#undef QT_FD
#undef QT_FS
#undef QT_FO
#undef QT_FI

        constexpr int kQtSentinelHi = (int)0xFFE00000; // -2^1023 * 1.x: below every down-dated norm, finite whatever the low word

        /// Slot retirement (lqr_qtol_body.inc, RETIRE): true when some level of a batch of full-rank levels of MD rows starts at a column Fc whose
        /// place is the LAST lane of slot NS - 2 — the level then starts with two live slots, the lower one holding one live column per problem.
        /// Instantiations for which no such level exists do not carry the path.
        constexpr bool qt_retire_reachable(int NS, int MD, int SIG, int NV)
        {
            for (int k = 1; k < kQuadMaxObj; k++)
            {
                const int fc = k * MD;
                if (fc < NV && ((fc + SIG) & 15) == 15 && ((fc + SIG) >> 4) == NS - 2) return true;
            }
            return false;
        }

        /// The elimination's ring of image rows (lqr_qtol_body.inc, RING_D / RING_W): how many steps in front of its use the U' row of a
        /// finished pivot is requested.  A step with one or two live slots (v_fmac_f64_dpp, 12 to 24 instructions) issues in less time than an
        /// LDS round trip takes, so one step of look-ahead leaves most of the trip to be waited for: three steps cover it.  A step with more
        /// live slots issues for about as long as the trip takes: two steps.  An entry costs two registers per live slot, eighteen at the
        /// most, held inside the elimination only.  (In the product kernel as compiled now the wide steps do not get their two steps: the
        /// compiler sinks their reads, with v_perm and address, to the head of the step that uses them — only the two broadcasts stay two
        /// steps in front; profiles/r09_qtol_elim_ring.md.  The steps with one or two live slots keep their reads where they are written.)
        /// Registers: the ring is live inside the elimination only (the register peak of every instantiation is in the pivot steps).  The estimating
        /// instantiations keep the one-ahead fetch: <3,12,7,40> and <3,12,0,0> of them have no register to spare.
        constexpr int qt_elim_ring_dpp(int NS, int MD, bool EST, bool RAG) { return EST ? 0 : 3; }
        constexpr int qt_elim_ring_wide(int NS, int MD, bool EST, bool RAG) { return EST ? 0 : 2; }
        /// ... of pivot position P: by the live slots of its step
        constexpr int qt_elim_ahead(int ring_dpp, int ring_wide, int NS, int SIG, int P) { return NS - (P + SIG) / 16 <= 2 ? ring_dpp : ring_wide; }

        /// NV: the number of variables when the instantiation serves ONE n (0: taken from the arguments) — the piece counts of the level loads and
        /// the layout tests then fold at compile time.
        /// EST: the accuracy guard's instantiation (lexls_lse_set_accuracy_guard).  Per problem it writes est_out[b] = the maximum over its
        /// pivots of |raw column| / |R_jj|: the norm of the pivot column in its level's rows as loaded (before the elimination by the levels
        /// above) over the diagonal the Householder step leaves.  A ratio far above one means that the level's rows lost most of that column
        /// to cancellation (elimination by near-dependent earlier pivots, down-dating within the level), which is where this kernel's
        /// summation order can move x beyond the tolerance contract.  Cost: MD fma per slot and level (column sums of squares of the block
        /// as staged) and a select / multiply / max per pivot step, off the decision chain; one double store per problem.  It also clears
        /// *count_reset (the flagged-problem counter of the compaction kernel that follows in the stream).  Without EST none of it exists.
        template <int NS, int MD, int SIG, int NV>
        __global__ __launch_bounds__(64 * QT_WPB) void lqr_qtol_kernel(LseArgs a, uint32_t img_doubles, uint32_t group_bytes, uint32_t stagger)
        {
            constexpr bool EST           = false;
            constexpr bool RAG           = false;
            double *const est_out        = nullptr;
            uint32_t *const count_reset  = nullptr;
#include "lqr_qtol_body.inc"
        }

        /// RAG: the ragged instantiation (lexls_lse_set_kernel_policy(h, 10)): level k of problem b has a.dims[b][k] <= MD rows, packed (its first
        /// row is the sum of the dimensions in front of it, as everywhere in the library).  The level block is the level with MD - d zero rows
        /// appended: a zero row adds nothing to a norm, a tail sum or a dot product and stays zero under the Gauss step and the rank-one update,
        /// so pivots, ranks and x are those of the level itself (tests/test_ragged_padding_oracle.py pins this on the oracle).  What differs
        /// from the uniform body: the level's first row is per problem (per-lane offsets of the level loads instead of a scalar base), rows
        /// d .. MD-1 are replaced by zeros after the load (select, not multiply: the memory behind a level holds the next level, slack, the next
        /// column), the loads are clamped to the column, and a level stops after d pivots whatever the tolerance.  The 16-byte loads sit at
        /// 8-byte alignment when a level starts at an odd row (or cap is odd): global memory accesses need no more than dword alignment in the
        /// unaligned access mode the HSA runtime runs kernels in (the compiler itself emits global_load_dwordx4 for an 8-byte aligned qt_d2u);
        /// the LDS side keeps its 16 bytes.
        template <int NS, int MD, int SIG, int NV>
        __global__ __launch_bounds__(64 * QT_WPB) void lqr_qtol_rag_kernel(LseArgs a, uint32_t img_doubles, uint32_t group_bytes, uint32_t stagger)
        {
            constexpr bool EST           = false;
            constexpr bool RAG           = true;
            double *const est_out        = nullptr;
            uint32_t *const count_reset  = nullptr;
#include "lqr_qtol_body.inc"
        }

        /// the accuracy guard's instantiation: the same body with EST (est_out: batch doubles; *count_reset is cleared).  The body is one text
        /// included twice rather than a function both kernels inline: the inlined form does not compile the shipped kernel to the same code
        template <int NS, int MD, int SIG, int NV>
        __global__ __launch_bounds__(64 * QT_WPB) void lqr_qtol_est_kernel(LseArgs a, uint32_t img_doubles, uint32_t group_bytes, uint32_t stagger, double *est_out,
                                                                          uint32_t *count_reset)
        {
            constexpr bool EST = true;
            constexpr bool RAG = false;
            if constexpr (NS == 3 && MD == 12 && NV == 0)
            {
#include "lqr_qtol_body_unpeeled.inc" // (the single-loop shape: this instantiation spills vector registers on the peeled body's lambdas)
            }
            else
            {
#include "lqr_qtol_body.inc"
            }
        }

        template <int NS, int MD, int SIG, int NV, bool EST = false, bool RAG = false>
        hipError_t launch_qtol_t(const LseArgs &a, hipStream_t s, double *est_out = nullptr, uint32_t *count_reset = nullptr)
        {
            static_assert(!(EST && RAG), "no estimating ragged form");
            const void *kfn;
            if constexpr (RAG)
                kfn = reinterpret_cast<const void *>(lqr_qtol_rag_kernel<NS, MD, SIG, NV>);
            else if constexpr (EST)
                kfn = reinterpret_cast<const void *>(lqr_qtol_est_kernel<NS, MD, SIG, NV>);
            else
                kfn = reinterpret_cast<const void *>(lqr_qtol_kernel<NS, MD, SIG, NV>);
            const uint32_t img  = qtol_image_doubles(a.nVar, a.nObj, MD);
            const size_t gbytes = qtol_group_bytes<NS, MD>(a.nVar, a.nObj);
            const size_t lds    = qtol_lds_bytes<NS, MD>(a.nVar, a.nObj);
            if (lds > kMaxLdsBytes || a.nObj > (uint32_t)kQuadMaxObj || a.nVar + 1 + SIG > 16u * NS || a.nVar > 63u || (NV && a.nVar != (uint32_t)NV)) return hipErrorInvalidValue;
            if ((reinterpret_cast<uintptr_t>(a.in) & (RAG ? 7u : 15u)) || a.nfixed || a.reg_type != 0) return hipErrorInvalidValue; // (RAG: its 16-byte loads are 8-byte aligned anyway)
            if (RAG ? (a.cap < 2u || !a.dims) : (a.uniform_dim != (uint32_t)MD || (a.cap & 1u))) return hipErrorInvalidValue; // (RAG: the caller vouches for dims <= MD; the kernel clamps)
            if (lds > 64 * 1024)
            {
                static size_t granted[64] = {0}; // per device: the attribute is set once, not per launch
                int dev = 0;
                if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
                if (dev < 0 || granted[dev] < lds)
                {
                    hipError_t e = hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                    if (e != hipSuccess) return e;
                    if (dev >= 0) granted[dev] = lds;
                }
            }
            const uint32_t blocks = (a.batch + 4u * QT_WPB - 1u) / (4u * QT_WPB);
            static const uint32_t stagger = std::getenv("LEXLS_QTOL_STAGGER") ? (uint32_t)std::atoi(std::getenv("LEXLS_QTOL_STAGGER")) : 0u; // x 512 cycles per SIMD index
            if constexpr (RAG)
                hipLaunchKernelGGL((lqr_qtol_rag_kernel<NS, MD, SIG, NV>), dim3(blocks), dim3(64 * QT_WPB), lds, s, a, img, (uint32_t)gbytes, stagger);
            else if constexpr (EST)
                hipLaunchKernelGGL((lqr_qtol_est_kernel<NS, MD, SIG, NV>), dim3(blocks), dim3(64 * QT_WPB), lds, s, a, img, (uint32_t)gbytes, stagger, est_out, count_reset);
            else
                hipLaunchKernelGGL((lqr_qtol_kernel<NS, MD, SIG, NV>), dim3(blocks), dim3(64 * QT_WPB), lds, s, a, img, (uint32_t)gbytes, stagger);
            return hipGetLastError();
        }
    } // namespace
} // namespace lexls

#define LEXLS_QTOL_INSTANCE(NAME, NS, MD, SIG, NV) \
    namespace lexls { hipError_t NAME(const LseArgs &a, hipStream_t s) { return launch_qtol_t<NS, MD, SIG, NV>(a, s); } }
// the accuracy guard's instantiation: est_out (batch doubles) receives the estimate, *count_reset is cleared
#define LEXLS_QTOL_INSTANCE_EST(NAME, NS, MD, SIG, NV) \
    namespace lexls { hipError_t NAME(const LseArgs &a, hipStream_t s, double *est_out, uint32_t *count_reset) { return launch_qtol_t<NS, MD, SIG, NV, true>(a, s, est_out, count_reset); } }
// the ragged instantiation (levels of up to MD rows, per-problem dimensions); its LDS is that of the uniform instantiation of the shape
#define LEXLS_QTOL_INSTANCE_RAG(NAME, NS, MD, SIG, NV) \
    namespace lexls { hipError_t NAME(const LseArgs &a, hipStream_t s) { return launch_qtol_t<NS, MD, SIG, NV, false, true>(a, s); } }

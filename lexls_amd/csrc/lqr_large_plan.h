// The host-side plan of the large path (lqr_large.hip): ONE place for its shape constants, the records the host sizes things by, the
// work-space layout of the step-per-pivot form, the pure half of the one-launch form's geometry and what is launched around a level.
// lqr_large.hip takes all of these from here; tests/large_plan_check.cpp prints them and tests/test_large_plan.py / test_large_cases.py
// check them on the CPU.  Plain host arithmetic, no device code: compiles with any C++17 compiler.
#pragma once
#include "lexls_lds.h"

#include <cstddef>
#include <cstdint>

#ifndef LEXLS_LARGE_TC
#define LEXLS_LARGE_TC 8 // trailing columns per apply-workgroup
#endif
#ifndef LEXLS_LARGE_NTP
#define LEXLS_LARGE_NTP 1024 // threads of the one-workgroup pivot kernel
#endif
#ifndef LEXLS_FAST_NW
#define LEXLS_FAST_NW 4 // wavefronts per workgroup of the step kernel
#endif
#ifndef LEXLS_FAST_CPW
#define LEXLS_FAST_CPW 1 // columns per wavefront of the step kernel
#endif
// the instantiated forms of the one-launch kernel: (wavefronts per workgroup, columns per wavefront)
#define LEXLS_PERSIST_FORMS(X) X(4, 1) X(4, 2) X(4, 4) X(8, 1) X(8, 2) X(16, 1)

namespace lexls
{
    namespace large
    {
        // ---- shape constants (types as the kernels use them) ----
        constexpr int TC = LEXLS_LARGE_TC;       // large_apply: trailing columns per workgroup
        constexpr int TJ = 8;                    // large_gemm: trailing columns per lane
        constexpr uint32_t NTP = LEXLS_LARGE_NTP; // large_pivot: threads; one trip of its loops covers NTP columns / rows
        constexpr int FNW = LEXLS_FAST_NW, FNT = 64 * FNW; // fast_step: wavefronts / threads per workgroup
        constexpr int FCPW = LEXLS_FAST_CPW;     // fast_step: columns per wavefront
        constexpr int FTC  = FNW * FCPW;         // fast_step: columns per workgroup
        constexpr int FRC  = 4;                  // fast_step: rows a lane keeps in registers between the dot product and the update (R <= 64 * FRC)
        constexpr int kStepCandWindow = 1024;    // fast_step: search candidates held in registers by the workgroup (n beyond it: a second loop reads again)
        constexpr int TRB = 8, TCH = 16;         // large_trsm_cols: rows per workgroup, multipliers per chunk
        constexpr uint32_t kTrsmColsMax = 1024;  // large_trsm_cols serves levels up to this dimension (a thread per column of the level), large_trsm beyond
        constexpr int GBM = 64, GBN = 64, GBK = 16; // large_gemm_mfma: output block and K step
        constexpr uint32_t kLevelEndRows = 1024; // fast_level_end: rows per block of the grid's x (256 threads, four trips)
        constexpr int PTC_MIN = 4;               // fewest columns per workgroup of LEXLS_PERSIST_FORMS: sizes the work space
        constexpr uint32_t kPersistMaxG = 256u;  // fast_level_persist: most workgroups (a poll keeps four records per lane of one wavefront in flight)
        constexpr uint32_t kRecNoPos  = 0xFFFFFu; // hand-off record: 20-bit position field, all ones = "no candidate"
        constexpr uint32_t kRecTagMax = 0xFFFFu;  // hand-off record: 16-bit tag field (pivot counter + 1)

        // ---- the records the host sizes things by ----
        struct LargeState
        {
            uint32_t ColIndex, rank, exhausted, F, dim, Fc, last_id, cur, piv, row, R, degenerate, totalrank, stop_level;
            double tau, diag, den;
        };
        struct PersistCtl
        {
            uint32_t arrive; // monotonic over the pivots of the level
            uint32_t abort;
            uint32_t done;   // workgroups that have finished every pivot of the level without giving up: the commit waits for all G
            uint32_t pad[13];
        };
        struct PersistCand
        {
            double norm;
            uint32_t pos, idx;
        };

        /// largest level dimension of the batch
        inline uint32_t max_level_dim(const uint32_t *level_max, uint32_t nObj)
        {
            uint32_t maxdim = 0;
            for (uint32_t k = 0; k < nObj; k++) maxdim = level_max[k] > maxdim ? level_max[k] : maxdim;
            return maxdim;
        }

        // ---- the one-launch form (fast_level_persist), pure half: what needs a device (occupancy, XCDs) stays in lqr_large.hip ----
        /// records per mailbox row (a reader's row starts on a 256-byte boundary); constexpr: the kernel calls it too
        constexpr size_t persist_mailbox_stride(uint32_t G) { return ((size_t)G + 15u) & ~(size_t)15u; }
        /// bytes of the two (pivot parity) sets of G mailbox rows
        inline size_t persist_mailbox_bytes(uint32_t G) { return 2 * (size_t)G * persist_mailbox_stride(G) * sizeof(PersistCand); }
        /// 16-byte granules of one published column: its rows + {fresh, tail} squared norms
        inline uint32_t persist_colld(uint32_t maxdim) { return (maxdim + 3u) & ~1u; }
        /// bytes of the two (pivot parity) sets of G published columns
        inline size_t persist_colbuf_bytes(uint32_t G, uint32_t maxdim) { return 16 * 2 * (size_t)G * persist_colld(maxdim); }
        /// dynamic LDS of a workgroup of ptc columns: tile, two pivot columns, the two position maps
        inline size_t persist_lds_bytes(int ptc, uint32_t n, uint32_t maxdim) { return 8 * ((size_t)ptc * (maxdim | 1u) + 2 * (size_t)maxdim) + 8 * (size_t)(n + 1); }
        /// workgroups of a form with ptc columns each (the right-hand side is column n)
        inline uint32_t persist_grid(uint32_t n, uint32_t ptc) { return (n + ptc) / ptc; }
        /// the record's position and tag fields hold every column position and every pivot of the level
        inline bool persist_fields_fit(uint32_t n, uint32_t maxdim) { return !(n + 1u >= kRecNoPos || maxdim >= kRecTagMax); }
        /// a form is worth asking the device about
        inline bool persist_within_limits(uint32_t G, size_t lds) { return !(lds > kMaxLdsBytes || G > kPersistMaxG); }

        // ---- work space of the step-per-pivot form: byte offsets from a base aligned to 64 bytes or more ----
        struct FastWorkspace
        {
            size_t W1;        // batch x cap x (n + 1) doubles: the second factor buffer
            size_t norms[2];  // batch x n doubles
            size_t D;         // batch x n doubles
            size_t E;         // batch x maxdim x maxdim doubles
            size_t st[2];     // batch LargeState
            size_t pos[2];    // batch x (n + 1) uint32_t
            size_t ctl;       // PersistCtl, 64-byte aligned
            size_t mailbox;   // persist_mailbox_bytes(Gmax)
            size_t colbuf;    // persist_colbuf_bytes(G, maxdim), G <= Gmax
            size_t total;     // end of the column buffer for Gmax
            uint32_t Gmax, colld;
            /// what is cleared in front of a one-launch level of G workgroups: [ctl, clear_end(G)) — the whole tail for G = Gmax
            size_t clear_end(uint32_t G) const { return colbuf + 16 * 2 * (size_t)G * colld; }
        };
        inline FastWorkspace fast_workspace_layout(uint32_t batch, uint32_t n, uint32_t cap, uint32_t maxdim)
        {
            FastWorkspace w;
            const size_t B = batch;
            size_t at      = 0;
            auto take      = [&](size_t bytes) {
                const size_t here = at;
                at += bytes;
                return here;
            };
            w.W1       = take(8 * B * cap * (n + 1));
            w.norms[0] = take(8 * B * n);
            w.norms[1] = take(8 * B * n);
            w.D        = take(8 * B * n);
            w.E        = take(8 * B * maxdim * maxdim);
            w.st[0]    = take(sizeof(LargeState) * B);
            w.st[1]    = take(sizeof(LargeState) * B);
            w.pos[0]   = take(4 * B * (n + 1));
            w.pos[1]   = take(4 * B * (n + 1));
            at         = (at + 63) & ~(size_t)63;
            w.Gmax     = persist_grid(n, PTC_MIN); // most workgroups of the one-launch forms
            w.colld    = persist_colld(maxdim);
            w.ctl      = take(sizeof(PersistCtl));
            w.mailbox  = take(persist_mailbox_bytes(w.Gmax));
            w.colbuf   = take(persist_colbuf_bytes(w.Gmax, maxdim));
            w.total    = at;
            return w;
        }

        // ---- dynamic LDS of the three multi-launch kernels that stage in LDS, for the largest level dimension of the batch ----
        struct LargeLds
        {
            size_t piv, app, trsm;
        };
        inline LargeLds large_lds_bytes(uint32_t n, uint32_t maxdim)
        {
            LargeLds l;
            l.piv  = 8 * ((size_t)((maxdim + 1) & ~1u) + NTP + 16) + 4 * (size_t)NTP;
            l.app  = 8 * ((size_t)TC * (maxdim | 1u) + maxdim + TC + 2);
            l.trsm = 8 * (size_t)((n < maxdim) ? n : maxdim) * 65;
            return l;
        }
        /// dynamic LDS of fast_step: the pivot column and its essential part
        inline size_t step_lds_bytes(uint32_t maxdim) { return 16 * (size_t)maxdim; }

        // ---- what is launched around level k, from (level_max[k], rows_max, n, last level) ----
        struct LevelPlan
        {
            bool gauss;              // a Gauss step runs below the level (an empty level has rank 0, the last level has nothing below)
            bool trsm_cols;          // large_trsm_cols (a thread per column of the level) instead of large_trsm (a row per lane)
            uint32_t trsm_grid;      // grid x of the TRSM taken
            uint32_t trsm_block;     // its threads
            uint32_t gemm_grid[2];   // grid x, y of large_gemm_mfma
            uint32_t level_end_grid; // grid x of fast_level_end
        };
        inline LevelPlan plan_level(uint32_t level_max, uint32_t rows_max, uint32_t n, bool last_level)
        {
            LevelPlan p;
            p.gauss     = !last_level && rows_max > 0 && level_max > 0;
            p.trsm_cols = level_max <= kTrsmColsMax;
            // the grids span the largest row count of the batch: workgroups beyond a problem's own rows return at once
            p.trsm_grid      = p.trsm_cols ? (rows_max + TRB - 1) / TRB : (rows_max + 63) / 64;
            p.trsm_block     = p.trsm_cols ? ((level_max + 63) / 64) * 64 : 64;
            p.gemm_grid[0]   = (rows_max + GBM - 1) / GBM;
            p.gemm_grid[1]   = (n + GBN) / GBN;
            p.level_end_grid = (rows_max + kLevelEndRows - 1) / kLevelEndRows;
            return p;
        }
    } // namespace large
    using large::LargeLds;
    using large::large_lds_bytes;
} // namespace lexls

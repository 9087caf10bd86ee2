// Body of lqr_qtol_kernel / lqr_qtol_est_kernel / lqr_qtol_rag_kernel (lqr_qtol_impl.h), included inside each: template parameters NS, MD, SIG, NV;
// arguments a, img_doubles, group_bytes, stagger; EST (constexpr bool), est_out, count_reset; RAG (constexpr bool): levels of up to MD rows.
// The phases of a level (head, staging, elimination, factor_level, level end) are local lambdas that take the level's block and the compile-time
// fact "this is level 0".  Level 0 is peeled: a straight-line section in front of the level loop on its own block blk0 (the direct load, identity
// layout, no staging, no elimination, factor_level<0>).  The loop runs the levels 1 .. nObj-1 on a block that is local to the iteration and first
// touched by the staging read: no value of a block is live into or out of an iteration, so none is carried round the back edge.
            static_assert(NS >= 1 && NS <= 4 && MD <= 16 && (MD % 4) == 0, "shape limits of the row layout / two row parts of even size");
            constexpr int NH  = 2;        // row parts of the staging transposition
            constexpr int RP  = MD / NH;  // rows per part
            constexpr int HP  = RP / 2;   // 16-byte pieces per column and part
            constexpr int kHandoffStride = 8 * MD + 16; // bytes between the lanes' hand-off slots: 16-byte aligned, b128 stores of 8 lanes on 32 banks
            constexpr int NIH = NS * HP;  // load instructions per part (16 NS columns x HP pieces / 16 lanes)
#ifndef LEXLS_QTOL_PF_STEPS
#define LEXLS_QTOL_PF_STEPS 9
#endif
            constexpr int PF_STEPS = LEXLS_QTOL_PF_STEPS < MD ? LEXLS_QTOL_PF_STEPS : MD; // pivot steps over which a level's requests are spread
            extern __shared__ double smem[];
            // LDS is addressed by 32-bit byte addresses turned into address-space-3 pointers directly (base of the dynamic block folded into the
            // slice offset once): an access through a generic pointer costs an extra add of the block's base (zero) per access
            typedef __attribute__((address_space(3))) char lds_char;
            const int lds0 = (int)(unsigned)(size_t)(lds_char *)smem;
            const int lane = threadIdx.x & 63;
            // QT_WPB wavefronts per workgroup (independent of each other; one per SIMD): a quarter of the workgroups to dispatch
            const uint32_t wq = QT_WPB > 1 ? blockIdx.x * QT_WPB + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : blockIdx.x; // this wavefront's quad of problems (in scalar registers)
            if (wq * 4u >= a.batch) return; // (a wavefront beyond the batch: nothing of it is waited for)
            if constexpr (EST)
            {
                if (wq == 0 && lane == 0) *count_reset = 0u;
            }
            const int g    = lane >> 4; // row = problem inside the wave
            const int gl   = lane & 15;
            const int n    = NV ? NV : (int)a.nVar;
            const int cap  = (int)a.cap;
            const int nObj = (int)a.nObj;
            const uint32_t b  = wq * 4u + (uint32_t)g;
            const uint32_t bb = b < a.batch ? b : a.batch - 1u; // rows beyond the batch idle on a valid address
            const bool live   = b < a.batch && !(a.skip && a.skip[bb]);
            const uint32_t pstride = (uint32_t)cap * (uint32_t)(n + 1);
            const double *inw      = a.in + (size_t)wq * 4u * pstride; // wave-uniform base; lane offsets stay 32-bit
            const uint32_t poff    = (bb - wq * 4u) * pstride;
            // (RAG) level k of this problem has (dpack >> 4 k) & 15 <= MD rows, packed: its first row is the sum of the levels in front (Frow).
            // Rows d .. MD-1 of a level block are zeros, whatever lies behind the level in memory: see lqr_qtol_impl.h
            uint32_t dpack = 0;
            int Frow       = 0;
            if constexpr (RAG)
            {
                static_assert(!EST && MD <= 15 && kQuadMaxObj <= 8, "four bits per level in one word; no estimating ragged form");
                const uint32_t dk = gl < nObj ? a.dims[(size_t)bb * (uint32_t)nObj + (uint32_t)gl] : 0u;
                const int dv      = (int)(dk < (uint32_t)MD ? dk : (uint32_t)MD);
                for_each_index<0, kQuadMaxObj>([&](auto kk) __attribute__((always_inline)) {
                    constexpr int k_ = decltype(kk)::value;
                    dpack |= (uint32_t)gbci<k_>(dv) << (4 * k_);
                });
            }
            // (RAG) the pair of rows R, R + 1 of a column is read at row min(R, cap - 2): no load leaves the column, so none leaves the input array.
            // R == cap - 1 (the column's last row, first of its pair) then arrives in the second half; rows from cap on belong to no level
            auto rag_rows = [&](qt_d2 v, int R, int r, int d, double &lo, double &hi) __attribute__((always_inline)) {
                lo = sel(r < d, sel(R == cap - 1, v.y, v.x), 0.0);
                hi = sel(r + 1 < d, v.y, 0.0);
            };

            // ---- the first level's rows are requested before anything else (every wave of the chip asks for its first level at once: the HBM serves
            //      this burst at its full rate, and nothing can be computed before it lands).  Its position layout is the identity, so lane = column
            //      loads the block directly, no staging; for such a burst this pattern is also the fastest of those measured
            //      (scripts/ubench/loadpat.hip: 7.7-8.4 k cycles per level against 9.5 k for the 48-byte pieces) ----
            double blk0[NS][MD]; // level 0's block, position layout (the later levels' blocks are local to the level loop's body)
#pragma unroll
            for (int s = 0; s < NS; s++)
            {
                const int P       = 16 * s + gl - SIG;
                const int c       = (P >= 0 && P <= n) ? P : 0;
                if constexpr (RAG)
                {
                    const double *colp = inw + (poff + (uint32_t)(c * cap));
                    const int d0       = (int)(dpack & 15u);
#pragma unroll
                    for (int r = 0; r < MD / 2; r++)
                    {
                        const int Rc  = 2 * r < cap - 2 ? 2 * r : cap - 2;
                        const qt_d2 v = *reinterpret_cast<const qt_d2u *>(colp + Rc); // (8-byte aligned when cap is odd)
                        rag_rows(v, 2 * r, 2 * r, d0, blk0[s][2 * r], blk0[s][2 * r + 1]);
                    }
                }
                else
                {
                    const qt_d2 *src2 = reinterpret_cast<const qt_d2 *>(inw + (poff + (uint32_t)(c * cap)));
#pragma unroll
                    for (int r = 0; r < MD / 2; r++)
                    {
                        const qt_d2 v      = src2[r];
                        blk0[s][2 * r]     = v.x;
                        blk0[s][2 * r + 1] = v.y;
                    }
                }
            }

            // ---- LDS carve-up of this row's slice (byte offsets; launch_qtol_t computes group_bytes) ----
            const int o_img   = lds0 + (int)((QT_WPB > 1 ? (threadIdx.x >> 6) * 4u : 0u) + (uint32_t)g) * (int)group_bytes;
            const int o_xs    = o_img + 8 * (int)img_doubles; // 16*NS : x by position (zero until the back-substitution: also the "U" of a position that is no pivot yet)
            const int o_ex    = o_xs + 8 * 16 * NS;           // MD    : dump slots (one dword per lane) of byte stores that do not apply
            const int o_phys  = o_ex + 8 * MD;                // 64 B  : physical column at each position
            const int o_perm  = o_phys + 64;                  // 64 B  : column_permutations
            const int o_meta  = o_perm + 64;                  // kQuadMaxObj x {first column, rank, image offset, image width}
            const int o_emap  = o_meta + 16 * kQuadMaxObj;    // 16 NS x 8 B: byte k of entry j = column index of PHYSICAL column j in the image of level k
            const int o_stage = o_emap + 8 * 16 * NS;         // max((n + 1) RP, 16 MD) doubles: staging block of the level loads; 16 hand-off slots of the pivot steps
            auto D   = [&](int off) -> __attribute__((address_space(3))) double & { return *(__attribute__((address_space(3))) double *)(size_t)(unsigned)off; };
            auto D2  = [&](int off) -> __attribute__((address_space(3))) qt_d2 & { return *(__attribute__((address_space(3))) qt_d2 *)(size_t)(unsigned)off; };
            auto B8  = [&](int off) -> __attribute__((address_space(3))) uint8_t & { return *(__attribute__((address_space(3))) uint8_t *)(size_t)(unsigned)off; };
            auto U32 = [&](int off) -> __attribute__((address_space(3))) uint32_t & { return *(__attribute__((address_space(3))) uint32_t *)(size_t)(unsigned)off; };
            auto U64 = [&](int off) -> __attribute__((address_space(3))) unsigned long long & { return *(__attribute__((address_space(3))) unsigned long long *)(size_t)(unsigned)off; };
            typedef unsigned qt_u4 __attribute__((ext_vector_type(4)));
            auto U4 = [&](int off) -> __attribute__((address_space(3))) qt_u4 & { return *(__attribute__((address_space(3))) qt_u4 *)(size_t)(unsigned)off; };

#pragma unroll
            for (int s = 0; s < 4; s++) B8(o_phys + 16 * s + gl) = (uint8_t)(16 * s + gl);
#pragma unroll
            for (int s = 0; s < NS; s++)
            {
                D(o_emap + 8 * (16 * s + gl)) = 0.0;
                D(o_xs + 8 * (16 * s + gl))   = 0.0;
            }
            quad_lds_fence();

            // The four waves of a CU (one per SIMD) start a little apart: every wave of the chip is in the same phase of the same level otherwise,
            // and each level's rows are asked for by all 1024 waves at once — a burst the HBM serves at its full rate while every SIMD waits
            if (stagger)
            {
                const unsigned simd = __builtin_amdgcn_s_getreg((4 << 0) | (4 << 6) | ((2 - 1) << 11)); // HW_REG_HW_ID, bits [5:4] = SIMD
                for (unsigned i = 0; i < simd * stagger; i++) __builtin_amdgcn_s_sleep(8);
            }

            // ---- level loads: pieces of 16 bytes, HP consecutive pieces = RP rows of one column, columns in consecutive lanes ----
            const int CH = (n + 1) * HP; // pieces per problem, level and row part
            static_assert(NH * NIH <= 18, "eighteen piece registers");
            // piece t = (row part t / NIH, instruction t % NIH) of the level whose first row is Frow -> its fixed registers
            // byte offsets of this lane's pieces inside a level, computed once (the division by HP is not repeated per request)
            uint32_t pieceoff[NH * NIH];
            for_each_index<0, NH * NIH>([&](auto tt) __attribute__((always_inline)) {
                constexpr int t = decltype(tt)::value, h = t / NIH, i = t % NIH;
                int ch        = 16 * i + gl;
                ch            = ch < CH ? ch : CH - 1; // lanes past the end repeat the last piece (same bytes to the same LDS address)
                const int col = ch / HP, m = ch - col * HP;
                if constexpr (RAG)
                    pieceoff[t] = ((uint32_t)(col * cap) << 2) | (uint32_t)m; // column offset in doubles and the pair inside the part: the row is per problem
                else
                    pieceoff[t] = 8u * (poff + (uint32_t)(col * cap + h * RP + 2 * m)); // bytes
            });
            static_assert(HP <= 4, "two bits for the pair index of a ragged piece");
            auto prefetch_piece = [&](auto tt, int Flev) __attribute__((always_inline)) { // Flev: first row of the level asked for
                constexpr int t = decltype(tt)::value, i = t % NIH;
                if (16 * i < CH) // wave-uniform
                {
                    if constexpr (RAG)
                    {
                        // the level's first row differs between the four problems of the wavefront: it goes into the lane's offset (clamped: rag_rows)
                        constexpr int h = t / NIH;
                        const int R     = Flev + h * RP + 2 * (int)(pieceoff[t] & 3u);
                        qt_pf_load<t>(inw, 8u * (poff + (pieceoff[t] >> 2) + (uint32_t)(R < cap - 2 ? R : cap - 2)));
                    }
                    else
                        qt_pf_load<t>(inw + Flev, pieceoff[t]);
                }
            };

            int rp[NS];         // slot s, lane l: LDS byte address of the (triangular) image row of pivot position c = 16 s + l - SIG
            int rq[NS];         // slot s, lane l: v_perm selector that picks the byte of pivot position c's LEVEL out of a column's index word
            unsigned long long em[NS]; // the index word of the column held in slot s
            int pos[NS];        // current position of the column held in slot s
            int pc[NS];         // its physical column
#pragma unroll
            for (int s = 0; s < NS; s++)
            {
                rp[s]  = o_xs; // (a position that is not a pivot yet "reads" zeros of the x block: see the elimination)
                rq[s]  = 0x0c0c0c00;
                em[s]  = 0ull;
                pos[s] = 0;
                pc[s]  = 0;
            }

            int ColIndex   = 0; // per row (uniform inside a row), like everything below
            int TotalRank  = 0;
            int imgoff     = 0; // doubles
            bool exh       = false;
            bool have_next = false; // the pieces of the level about to start are already in flight / in registers (wave-uniform)
            double est2    = 0.0;   // (EST) this lane's largest |raw column|^2 / (4 R_jj^2) over the pivots it held
            double rsq[NS];         // (EST) squared norm of the column in slot s over the level's rows as loaded (set at every level start)
            STAMP_DECL
            STAMP(0)
#ifdef LEXLS_QTOL_CHAIN
            unsigned long long cacc[7] = {0, 0, 0, 0, 0, 0, 0};
#endif
#ifdef LEXLS_WAVE_STAMPS
            unsigned long long lst_t0 = clock64();
#endif

            // ---- the phases of one level, as lambdas: each takes the level's block and (l0c) the compile-time fact "this is level 0", the peeled
            //      section in front of the level loop (L0: no look-ups, no staging, no elimination, k == 0; QT_LMARK names its parts "level0-...") ----
            // PEEL is off for the estimating instantiation with three slots of twelve rows (<3,12,7,40> with EST): peeled it spills four vector
            // registers (scripts/check_qtol_regs.py refuses that).  It keeps the single loop over all levels, the block carried round it, on the
            // same lambdas (never L0: the k > 0 tests are then run-time tests).  (<3,12,0,0> with EST spills two in either shape and is compiled
            // from lqr_qtol_body_unpeeled.inc: lqr_qtol_impl.h)
            constexpr bool PEEL = !(EST && NS == 3 && MD == 12);
            // RETIRE: a level that starts with two live slots, the lower of which (slot NS - 2) holds ONE live column per problem — the column at
            // position Fc, in lane 15; every other lane of the slot holds a finished pivot — drops that slot after its first pivot step.  The
            // columns of a level do not move, only pos[] swaps, so that one physical column would keep the whole slot in every pivot step until it
            // wins.  Behind step 0 the winner's register place is finished (what the level end stores of it is written then and there); the lone
            // column moves into that place through LDS with its norm, position and physical column (lane 15 writes, the winner's lane reads), and
            // the steps 1 .. MD-1 and the level end run on the upper slot alone.  No operand and no order of operations changes and positions are
            // unique in the decision key, so pivots, ranks and x are bit for bit those of the unretired level.  Taken only when all four problems
            // of the wavefront work and start the level at the same such column (hh-select); anything else takes factor_level<S0> as before.
            // Off (same code as without it) for the estimating and ragged forms, for an n known at run time only (the staging block has the
            // room for the move's 8 MD + 16 bytes behind the hand-off slots when (n + 1) RP doubles say so) and for shapes whose full-rank levels
            // never start at such a column (qt_retire_reachable).
            constexpr int kRetireSlot = NS - 2;
            constexpr bool RETIRE     = !EST && !RAG && PEEL && NV > 0 && qt_retire_reachable(NS, MD, SIG, NV) && 8 * (NV + 1) * RP >= 17 * kHandoffStride;
            // RING_D / RING_W: how many steps ahead the elimination requests a finished pivot's image row, for the steps with one or two live
            // slots / with more (qt_elim_ring_dpp, qt_elim_ring_wide in lqr_qtol_impl.h; 0: the one-ahead fetch, the instantiation's earlier code)
            constexpr int RING_D = qt_elim_ring_dpp(NS, MD, EST, RAG), RING_W = qt_elim_ring_wide(NS, MD, EST, RAG);
            static_assert((RING_D > 0) == (RING_W > 0), "a ring serves every step form of its instantiation");
            struct qt_level // what the phases of one level hand to each other (per row, uniform inside a row; prefetch: wave-uniform)
            {
                bool work;     // x only: once the columns are exhausted nothing below matters
                int F;         // first row of the level
                int dlev;      // its rows (RAG: per problem)
                int Fc;        // its first column
                int rank;
                bool prefetch; // the next level's rows are requested inside this level's pivot steps
            };

            // level head: false when no row of the wavefront has work left (the level's meta entry is written, nothing else of the level runs)
            auto level_head = [&](auto l0c, const int k, qt_level &L) __attribute__((always_inline)) {
                constexpr bool L0 = decltype(l0c)::value;
                QT_LMARK("level-top")
                L.work = live && !exh;
                L.F    = RAG ? Frow : k * MD;
                L.dlev = RAG ? (int)((dpack >> (4 * k)) & 15u) : MD;
                if constexpr (RAG) Frow += L.dlev;
                L.Fc   = ColIndex;
                L.rank = 0;
                if (__ballot(L.work) == 0ull)
                {
                    if (gl == 0)
                    {
                        U32(o_meta + 16 * k)      = (uint32_t)L.Fc;
                        U32(o_meta + 16 * k + 4)  = 0u;
                        U32(o_meta + 16 * k + 8)  = (uint32_t)imgoff;
                        U32(o_meta + 16 * k + 12) = (uint32_t)(n + 1 - L.Fc);
                    }
                    return false;
                }
                if constexpr (!L0)
                {
                    if ((PEEL || k > 0) && !have_next) // a level whose predecessor could have exhausted the columns: all pieces at once
                        for_each_index<0, NH * NIH>([&](auto tt) __attribute__((always_inline)) { prefetch_piece(tt, L.F); });
                }
                return true;
            };

            // =====================================================================================
            // position layout of the level; staged pieces -> block (levels behind level 0: every entry of blk is written here before anything reads it)
            // =====================================================================================
            auto level_start = [&](const int k, const qt_level &L, double (&blk)[NS][MD]) __attribute__((always_inline)) {
                const int F = L.F, dlev = L.dlev;
                (void)F, (void)dlev;
                QT_MARK("level-start")
#pragma unroll
                for (int s = 0; s < NS; s++)
                {
                    const int P  = 16 * s + gl - SIG;
                    const int ph = (int)B8(o_phys + (P >= 0 && P < n ? P : 0)); // (unconditional reads: the three slots' look-ups go out together)
                    pc[s]        = (P >= 0 && P < n) ? ph : (P == n ? n : 0);
                    pos[s]       = (P >= 0 && P <= n) ? P : 0x3fffff;
                }
#pragma unroll
                for (int s = 0; s < NS; s++) em[s] = U64(o_emap + 8 * pc[s]);
                if (PEEL || k > 0) // (the unpeeled shape: level 0's block came by the direct load)
                for_each_index<0, NH>([&](auto hh) __attribute__((always_inline)) {
                    constexpr int h = decltype(hh)::value;
                    QT_MARK1("level-stage", h)
                    // the pieces come out of their fixed registers (requested during the level in front, or just now)
                    if constexpr (h == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    for_each_index<0, NIH>([&](auto ii) __attribute__((always_inline)) {
                        constexpr int i = decltype(ii)::value;
                        if (16 * i < CH)
                        {
                            int ch = 16 * i + gl;
                            ch     = ch < CH ? ch : CH - 1;
                            qt_pf_store_lds<h * NIH + i>(o_stage + 16 * ch);
                        }
                    });
                    quad_lds_fence();
#pragma unroll
                    for (int s = 0; s < NS; s++)
                    {
#pragma unroll
                        for (int m = 0; m < HP; m++)
                        {
                            const qt_d2 v            = D2(o_stage + 16 * (pc[s] * HP + m));
                            if constexpr (RAG)
                                rag_rows(v, F + h * RP + 2 * m, h * RP + 2 * m, dlev, blk[s][h * RP + 2 * m], blk[s][h * RP + 2 * m + 1]);
                            else
                            {
                                blk[s][h * RP + 2 * m]     = v.x;
                                blk[s][h * RP + 2 * m + 1] = v.y;
                            }
                        }
                    }
                    quad_lds_fence();
                });
            };

            // behind the block's arrival: (EST) the raw column norms; whether the next level's rows are requested inside this level's pivot steps
            auto level_post = [&](auto l0c, const int k, qt_level &L, double (&blk)[NS][MD]) __attribute__((always_inline)) {
                constexpr bool L0 = decltype(l0c)::value;
                const bool work = L.work;
                const int Fc    = L.Fc;
                (void)k;
                STAMP(1)
                LSTAMP(0)
                QT_LMARK("level-post")
                if constexpr (EST)
                {
#pragma unroll
                    for (int s = 0; s < NS; s++)
                    {
                        double t = 0.0;
#pragma unroll
                        for (int r = 0; r < MD; r++) t = dfma(blk[s][r], blk[s][r], t);
                        rsq[s] = t;
                    }
                }
                // the next level's rows: requested while this level is factorised (two pieces per pivot step, below), unless this level can
                // exhaust the columns
                L.prefetch = (k + 1 < nObj) && (rows_min(work ? Fc : 0x3fffffff) + MD < n);
                have_next  = L.prefetch;
            };

            // =====================================================================================
            // Gauss elimination of these rows by every finished pivot c' (lexlse.h:431-471, left-looking, normalised pivot rows).  Level 0 has none
            // =====================================================================================
            auto eliminate = [&](const int k, const qt_level &L, double (&blk)[NS][MD]) __attribute__((always_inline)) {
                (void)k;
                const int Fcmax = rows_max(L.work ? L.Fc : 0);
                ESTAMP_DECL
                {
                    // U'[c'][P] of this lane's columns: one LDS read per live slot behind a row-broadcast address.  Everything it reads — rp, rq,
                    // the index words, the image rows of the finished levels — is final when the level starts
                    auto fetch_u = [&](auto cc, double (&u)[NS]) __attribute__((always_inline)) {
                        constexpr int C  = decltype(cc)::value;
                        constexpr int sc = (C + SIG) / 16, lc = (C + SIG) % 16;
                        const int rowp   = gbci<lc>(rp[sc]);
                        const int selq   = gbci<lc>(rq[sc]);
#pragma unroll
                        for (int s = sc; s < NS; s++)
                        {
                            const unsigned e = __builtin_amdgcn_perm((unsigned)(em[s] >> 32), (unsigned)em[s], (unsigned)selq);
                            u[s]             = D(rowp + (int)(e << 3));
                        }
                    };
                    constexpr int NP = 16 * NS - SIG; // pivot positions
                    if constexpr (RING_D > 0)
                    {
                    // The rows are kept in flight several steps ahead, in a ring of registers: the row of pivot P is requested qt_elim_ahead(P)
                    // steps in front of step P (at the level head when that is before step 0), into entry P % RD.  A step takes its entry and
                    // re-issues the entries of the pivots whose turn it is, in ascending order, behind the first use of its own: the LDS round
                    // trip of a row is covered by the fma issue of the steps in front instead of being waited for in every step.  Indices are
                    // compile-time constants, so every entry is a named register and the compiler counts the reads in flight itself
                    // (s_waitcnt lgkmcnt(N), N = the reads issued behind the step's own).  The requests are unconditional: a position beyond
                    // the problem's (or the wavefront's) finished pivots reads a zero of the x block, as such a position does in a step that
                    // runs for another row's sake, and what was asked for a step that does not run is not used.
                    constexpr int RD = RING_D > RING_W ? RING_D : RING_W;
                    double ring[RD][NS];
                    for_each_index<0, (RD < NP ? RD : NP)>([&](auto pp) __attribute__((always_inline)) {
                        constexpr int P = decltype(pp)::value;
                        if constexpr (P < qt_elim_ahead(RING_D, RING_W, NS, SIG, P)) fetch_u(pp, ring[P % RD]);
                    });
                    ESTAMP(0)
                    qt_for_each_while<0, NP>(
                        [&](auto cc) __attribute__((always_inline)) { return decltype(cc)::value < Fcmax; }, // wave-uniform
                        [&](auto cc) __attribute__((always_inline)) {
                            constexpr int C  = decltype(cc)::value;
                            constexpr int sc = (C + SIG) / 16, lc = (C + SIG) % 16;
                            if constexpr (C > 0 && lc == 0) { ESTAMP(NS - sc + 1) } // (the form in front ends here)
                            QT_MARK1("elim", C)
                            double ucur[NS];
#pragma unroll
                            for (int s = sc; s < NS; s++) ucur[s] = ring[C % RD][s];
                            auto refill = [&]() __attribute__((always_inline)) {
                                for_each_index<C + 1, (C + RD + 1 < NP ? C + RD + 1 : NP)>([&](auto pp) __attribute__((always_inline)) {
                                    constexpr int P = decltype(pp)::value;
                                    if constexpr (P - qt_elim_ahead(RING_D, RING_W, NS, SIG, P) == C) fetch_u(pp, ring[P % RD]);
                                });
                            };
                            if constexpr (NS - sc <= 2)
                            {
                                if constexpr (sc + 1 < NS) qt_gauss_dpp<lc>(blk[sc + 1], blk[sc], ucur[sc + 1]);
                                refill();
                                qt_gauss_dpp_self<lc>(blk[sc], ucur[sc]);
                            }
                            else
                            {
                                double lr[MD];
                                for_each_index<0, MD>([&](auto rr) {
                                    constexpr int r = decltype(rr)::value;
                                    lr[r]           = gbc<lc>(blk[sc][r]);
                                });
#pragma unroll
                                for (int r = 0; r < MD; r++) blk[sc][r] = dfma(-lr[r], ucur[sc], blk[sc][r]);
                                refill();
#pragma unroll
                                for (int s = sc + 1; s < NS; s++)
                                {
#pragma unroll
                                    for (int r = 0; r < MD; r++) blk[s][r] = dfma(-lr[r], ucur[s], blk[s][r]);
                                }
                            }
                        });
                    }
                    else
                    {
                    // (no ring in this instantiation: the row is fetched one pivot ahead of its use)
                    double ua[NS], ub[NS]; // even / odd steps (no copies between the steps)
#pragma unroll
                    for (int s = 0; s < NS; s++) ua[s] = ub[s] = 0.0;
                    if (Fcmax > 0) fetch_u(std::integral_constant<int, 0>{}, ua);
                    ESTAMP(0)
                    qt_for_each_while<0, NP>(
                        [&](auto cc) __attribute__((always_inline)) { return decltype(cc)::value < Fcmax; }, // wave-uniform
                        [&](auto cc) __attribute__((always_inline)) {
                            constexpr int C  = decltype(cc)::value;
                            constexpr int sc = (C + SIG) / 16, lc = (C + SIG) % 16;
                            double(&ucur)[NS]  = (C & 1) ? ub : ua;
                            double(&unext)[NS] = (C & 1) ? ua : ub;
                            if constexpr (C > 0 && lc == 0) { ESTAMP(NS - sc + 1) } // (the form in front ends here)
                            QT_MARK1("elim", C)
                            // a row of the wavefront whose own pivots end before Fcmax meets the zeros of the x block as "U'": every fma adds a zero product
                            if constexpr (NS - sc <= 2)
                            {
                                // one or two slots left: the broadcast of l rides in the fma (qt_gauss_dpp: MD instructions per slot, no moves).  The
                                // slot behind first — it reads the l of the pivot's slot, whose own update (last) turns lane lc into zero
                                if constexpr (sc + 1 < NS) qt_gauss_dpp<lc>(blk[sc + 1], blk[sc], ucur[sc + 1]);
                                if constexpr (C + 1 < 16 * NS - SIG)
                                {
                                    if (C + 1 < Fcmax) fetch_u(std::integral_constant<int, C + 1>{}, unext);
                                }
                                qt_gauss_dpp_self<lc>(blk[sc], ucur[sc]);
                            }
                            else
                            {
                                double lr[MD];
                                for_each_index<0, MD>([&](auto rr) {
                                    constexpr int r = decltype(rr)::value;
                                    lr[r]           = gbc<lc>(blk[sc][r]);
                                });
#pragma unroll
                                for (int r = 0; r < MD; r++) blk[sc][r] = dfma(-lr[r], ucur[sc], blk[sc][r]);
                                // (the next step's U' behind the first slot's work: its address chain does not stall the step's start)
                                if constexpr (C + 1 < 16 * NS - SIG)
                                {
                                    if (C + 1 < Fcmax) fetch_u(std::integral_constant<int, C + 1>{}, unext);
                                }
#pragma unroll
                                for (int s = sc + 1; s < NS; s++)
                                {
#pragma unroll
                                    for (int r = 0; r < MD; r++) blk[s][r] = dfma(-lr[r], ucur[s], blk[s][r]);
                                }
                            }
                        });
                    }
                    ESTAMP_END(Fcmax)
                    // (what follows may read the block through DPP: the wait states behind the last block's writes, which the compiler does not count.
                    //  Here, once per level, and not at the end of qt_gauss_dpp_self, where it would be paid in every step: between the steps the
                    //  next block's own leading s_nop serves.  A level without a folded step pays two idle cycles)
                    asm volatile("s_nop 1");
                }
                STAMP(7)
                LSTAMP(1)
            };

                // =====================================================================================
                // Householder QR with column pivoting of the level (lexlse.h:182-268), slots S0 .. NS-1.
                // Straight-line per pivot, ONE basic block: a row that has stopped keeps executing on data nobody reads again, its bookkeeping
                // frozen by selects.  Order inside a step = the dependency chain, with everything that is not on it placed in its shadows:
                //   read the pivot column (LDS, slot of the winning lane)  ->  tail / fresh norm  ->  1/sqrt  ->  row j of the block,
                //   down-dated norms  ->  DECISION for pivot j+1 (local best, two butterflies)  ->  next read.
                // Beside the chain: the raw dot products (beside the 1/sqrt), the reciprocal of c0 - beta and the rank-one update of the rows
                // below (beside the butterflies), then every lane stores the column of its local best slot in its own LDS slot — the store
                // does not wait for the decision, only the next step's read address does.
                // =====================================================================================
                // retc (RETIRE): slot S0 is dropped behind pivot step 0 — steps 1 .. MD-1 run on the slots S0 + 1 .. NS-1 (k: the level, for the
                // winner's index byte)
                auto factor_level = [&](auto l0c, auto s0c, auto retc, const int k, qt_level &L, double (&blk)[NS][MD]) __attribute__((always_inline)) {
                    constexpr bool L0 = decltype(l0c)::value;
                    constexpr int S0 = decltype(s0c)::value;
                    constexpr bool RET = decltype(retc)::value;
                    constexpr int SL = NS - S0; // live slots
                    static_assert(!L0 || S0 == 0, "level 0 starts at column 0: every slot is live");
                    static_assert(!RET || (RETIRE && !L0 && S0 == kRetireSlot && SL == 2), "the retiring form: two live slots, one behind step 0");
                    (void)k;
                    const bool work = L.work, prefetch = L.prefetch;
                    const int F = L.F, dlev = L.dlev;
                    int &rank = L.rank;
                    if constexpr (RET) { QT_MARK1("hh-ret-pro", S0) } else { QT_LMARK1("hh-pro", S0) }
                    double nrm[NS];
#pragma unroll
                    for (int s = S0; s < NS; s++)
                    {
                        double t = 0.0;
#pragma unroll
                        for (int r = 0; r < MD; r++) t = dfma(blk[s][r], blk[s][r], t); // lexlse.h:193-196
                        nrm[s] = sel(pos[s] >= ColIndex && pos[s] < n, t, qt_with_hi(t, kQtSentinelHi));
                    }
                    bool go = work;
#ifdef LEXLS_QTOL_CHAIN
                    unsigned long long ct[7] = {0, 0, 0, 0, 0, 0, 0}, cp1 = 0;
                    bool cvalid = false;
#endif
                    // Pivot decision: first maximum (by position) of the down-dated norms (lexlse.h:205-206) as ONE f64 max butterfly: the low twelve
                    // bits of a candidate's norm are replaced by 4095 - (position << 6 | slot << 4 | lane) for the comparison, so that equal
                    // norms order by position and the winner's identity comes out of the maximum itself.  (Norms that agree in their upper
                    // 52 - 12 mantissa bits also order by position: a 2^-40 window in which the reference's own choice depends on its summation
                    // order.  The norms themselves stay untouched.)
                    int cur_lbs = S0, nxt_lbs = S0;     // slot of the lane's local best candidate: for this pivot / the next one
                    bool cur_ispl = false, nxt_ispl = false; // this lane holds the pivot column
                    unsigned cur_w = 0, nxt_w = 0;      // the winner's 12-bit key (position << 6 | slot << 4 | lane)
                    double pbest = 0.0;                 // the lane's local best, packed
                    auto decide_local = [&](auto loc) __attribute__((always_inline)) { // loc: the lowest live slot
                        constexpr int LO = decltype(loc)::value;
#pragma unroll
                        for (int s = LO; s < NS; s++)
                        {
                            const int kinv  = (0xFFF - ((s << 4) | gl)) - (pos[s] << 6);
                            const double pv = __hiloint2double(__double2hiint(nrm[s]), (__double2loint(nrm[s]) & ~0xFFF) | kinv);
                            pbest           = s == LO ? pv : vmax(pbest, pv);
                        }
                        nxt_lbs = ((0xFFF - (__double2loint(pbest) & 0xFFF)) >> 4) & 3;
                    };
                    auto decide_finish = [&](double m) __attribute__((always_inline)) {
                        const int mlo = __double2loint(m);
                        nxt_w         = (unsigned)(0xFFF - (mlo & 0xFFF));
                        nxt_ispl      = ((__double2loint(pbest) ^ mlo) & 0xFFF) == 0;
                    };
                    // prologue: decision for pivot 0, every lane's best column to its hand-off slot
                    {
                        decide_local(std::integral_constant<int, S0>{});
                        decide_finish(row_max16(pbest));
                        double colv[MD];
#pragma unroll
                        for (int r = 0; r < MD; r++) colv[r] = blk[S0][r];
#pragma unroll
                        for (int s = S0 + 1; s < NS; s++)
                        {
                            const bool pick = nxt_lbs == s;
#pragma unroll
                            for (int r = 0; r < MD; r++) colv[r] = sel(pick, blk[s][r], colv[r]);
                        }
#pragma unroll
                        for (int r = 0; r < MD; r += 2) D2(o_stage + gl * kHandoffStride + 8 * r) = qt_d2{colv[r], colv[r + 1]};
                        cur_lbs = nxt_lbs, cur_ispl = nxt_ispl, cur_w = nxt_w;
                    }
                    // the winner's column is read AHEAD: as soon as a step knows the next pivot's lane, the read is issued — the rest of the step (rank-one
                    // update of the other columns) runs while it is on its way
                    double coln[MD];
                    auto fetch_column = [&](auto jjc, unsigned w) __attribute__((always_inline)) {
                        constexpr int ce0 = decltype(jjc)::value & ~1;
                        quad_lds_fence();
                        const int src = o_stage + (int)(w & 15u) * kHandoffStride;
#pragma unroll
                        for (int r = ce0; r < MD; r += 2)
                        {
                            const qt_d2 v   = D2(src + 8 * r);
                            coln[r]         = v.x;
                            coln[r + 1]     = v.y;
                        }
                    };
                    fetch_column(std::integral_constant<int, 0>{}, cur_w);

                    int pf_issued = 0; // pieces of the next level requested so far (wave-uniform)
                    qt_for_each_while<0, MD>(
                        [&](auto jc) __attribute__((always_inline)) { return (decltype(jc)::value % 4 != 0) || __ballot(go) != 0ull; }, // tested every fourth step: no row of the wavefront has work left -> ONE branch leaves the level
                        [&](auto cnt) __attribute__((always_inline)) {
                        constexpr int j   = decltype(cnt)::value;
                        constexpr int ce  = j & ~1;       // first (even) row of this step's hand-off
                        constexpr int cen = (j + 1) & ~1; // ... of the next step's
                        constexpr int SJ  = (RET && j >= 1) ? S0 + 1 : S0; // lowest live slot of this step
                        constexpr int SLJ = NS - SJ;
                        if constexpr (RET) { QT_MARK2("hh-ret-step", S0, j) } else { QT_LMARK2("hh-step", S0, j) }
                        // (RET) the pivot of step 0, for the move behind it
                        const unsigned w0 = cur_w;
                        const bool ispl0  = cur_ispl;
                        (void)w0, (void)ispl0;
                        // the next level's pieces: PF_PER per pivot step from the first step on (what an early end leaves over is requested behind the loop)
                        {
                            constexpr int TOT = NH * NIH, PF_PER = (TOT + PF_STEPS - 1) / PF_STEPS;
                            constexpr int lo = (j * PF_PER < TOT ? j * PF_PER : TOT), hi = ((j + 1) * PF_PER < TOT ? (j + 1) * PF_PER : TOT);
                            if (prefetch) for_each_index<lo, hi>([&](auto tt) __attribute__((always_inline)) { prefetch_piece(tt, F + dlev); });
                            pf_issued = hi;
                        }
                        const bool act = go;
                        CSTAMP(0, (int)cur_w)
                        double col[MD];
#pragma unroll
                        for (int r = ce; r < MD; r++) col[r] = coln[r];
                        FSTAMP(2)
                        CSTAMP(1, __double2loint(col[MD - 1]))
                        CSTAMP_COLLECT
                        const double c0 = col[j];
                        // tail norm in three partial sums, fresh norm = c0^2 + tail (lexlse.h:210-211, :241)
                        double t0 = 0.0, t1 = 0.0, t2 = 0.0;
#pragma unroll
                        for (int r = j + 1; r < MD; r++)
                        {
                            if ((r - j) % 3 == 1) t0 = dfma(col[r], col[r], t0);
                            if ((r - j) % 3 == 2) t1 = dfma(col[r], col[r], t1);
                            if ((r - j) % 3 == 0) t2 = dfma(col[r], col[r], t2);
                        }
                        const double tailSq = (t0 + t1) + t2;
                        const double fresh  = dfma(c0, c0, tailSq);
                        CSTAMP(2, __double2loint(fresh))
                        // rank test on the squared norm (lexlse.h:214); no branch: a stopped row runs on.  (RAG) a level ends with its own rows, whatever
                        // the tolerance: behind them the column is exactly zero
                        const bool cont     = RAG ? (act && !(fresh < a.tol) && j < dlev) : (act && !(fresh < a.tol));
                        go                  = cont;
                        // 1 / sqrt(fresh): v_rsq_f64 and two coupled iterations (g -> sqrt, h -> 1 / (2 sqrt))
                        double g, h;
                        {
                            const double y = __builtin_amdgcn_rsq(fresh);
                            g              = fresh * y;
                            h              = 0.5 * y;
                            double r       = dfma(-h, g, 0.5);
                            g              = dfma(g, r, g);
                            h              = dfma(h, r, h);
#ifndef LEXLS_QTOL_ONE_NEWTON
                            r              = dfma(-h, g, 0.5);
                            g              = dfma(g, r, g);
                            h              = dfma(h, r, h);
#endif
                        }
                        const bool neg    = c0 >= 0.0;       // beta = -sign(c0) sqrt(fresh)
                        const double beta = neg ? -g : g;
                        const double ibet = (neg ? -2.0 : 2.0) * h; // 1 / beta
                        CSTAMP(3, __double2loint(ibet))
                        const double rden = qt_rcp1(c0 - beta);     // (for the rows below; not on the chain to the next decision)
                        // raw dot products col . a of every live column (beside the chain above)
                        double dw[NS];
#pragma unroll
                        for (int s = SJ; s < NS; s++)
                        {
                            double d0 = 0.0, d1 = 0.0;
#pragma unroll
                            for (int r = j + 1; r < MD; r++)
                            {
                                if ((r - j) & 1)
                                    d0 = dfma(col[r], blk[s][r], d0);
                                else
                                    d1 = dfma(col[r], blk[s][r], d1);
                            }
                            dw[s] = dfma(c0, blk[s][j], d0 + d1);
                        }
                        FSTAMP(3)
                        // row j of the block: R_js = (col . a_s) / beta (final after this reflector); norm down-date (lexlse.h:262-266); the pivot
                        // column leaves the candidates; the row is kept normalised by 1 / R_jj.  gs: a_s[r] += gs col[r] for the rows below,
                        // gs = (R_js - a_s[j]) / (c0 - beta)   (= a_s - tau v v.a_s, lexlse.h:243-246)
                        double gs[NS];
#pragma unroll
                        for (int s = SJ; s < NS; s++)
                        {
                            const double t = dw[s] * ibet;
                            gs[s]          = (t - blk[s][j]) * rden;
                            nrm[s]         = dfma(-t, t, nrm[s]);
                            nrm[s]         = sel(cont && cur_ispl && cur_lbs == s, qt_with_hi(nrm[s], kQtSentinelHi), nrm[s]);
                            blk[s][j]      = t * ibet;
                        }
                        CSTAMP(4, __double2hiint(nrm[NS - 1]))
                        // column "swap": update the position map (lexlse.h:222-232)
                        const int ppos = (int)(cur_w >> 6);
#pragma unroll
                        for (int s = SJ; s < NS; s++)
                        {
                            const bool front = cont && pos[s] == ColIndex;
                            pos[s]           = sel(front, ppos, pos[s]);
                            pos[s]           = sel(cont && cur_ispl && cur_lbs == s, ColIndex, pos[s]);
                        }
                        B8(sel(cont && cur_ispl, o_perm + ColIndex, o_ex + 4 * gl)) = (uint8_t)ppos; // (o_ex: dump slots, one bank per lane — same-address stores of many lanes serialise)
                        if constexpr (EST)
                        {
                            // the pivot's lane: its raw squared norm times h^2 = 1 / (4 fresh)
                            double r2 = rsq[SJ];
#pragma unroll
                            for (int s = SJ + 1; s < NS; s++) r2 = sel(cur_lbs == s, rsq[s], r2);
                            est2 = sel(cont && cur_ispl, vmax(est2, r2 * (h * h)), est2);
                        }
                        ColIndex += cont ? 1 : 0;
                        rank += cont ? 1 : 0;
                        const bool full = cont && ColIndex == n;
                        exh             = exh || full;
                        go              = go && !full;
                        FSTAMP(4)
                        if constexpr (j + 1 < MD && SLJ == 1)
                        {
                            // one live slot: the lane's best column IS the slot — update it (in the stalls of the butterfly), store it
                            decide_local(std::integral_constant<int, SJ>{});
                            double m = pbest;
                            auto upd_rows = [&](auto qq) __attribute__((always_inline)) {
                                constexpr int q = decltype(qq)::value;
#pragma unroll
                                for (int r = j + 1; r < MD; r++)
                                    if ((r - j - 1) % 4 == q) blk[SJ][r] = dfma(gs[SJ], col[r], blk[SJ][r]);
                            };
                            m = dpp_max<0xB1>(m);
                            upd_rows(std::integral_constant<int, 0>{});
                            m = dpp_max<0x4E>(m);
                            upd_rows(std::integral_constant<int, 1>{});
                            m = dpp_max<0x141>(m);
                            upd_rows(std::integral_constant<int, 2>{});
                            m = dpp_max<0x140>(m);
                            upd_rows(std::integral_constant<int, 3>{});
#pragma unroll
                            for (int r = cen; r < MD; r += 2) D2(o_stage + gl * kHandoffStride + 8 * r) = qt_d2{blk[SJ][r], blk[SJ][r + 1]};
                            decide_finish(m);
                            fetch_column(std::integral_constant<int, j + 1>{}, nxt_w);
                        }
                        else if constexpr (j + 1 < MD)
                        {
                            // The decision for the next pivot: local part, then the four butterfly stages.  In the stalls of the stages: the lane's
                            // best column (for the next hand-off) is picked out of the slots BEFORE the rank-one update, updated on its own and
                            // stored — the store does not wait for the decision, only the next step's read address does
                            decide_local(std::integral_constant<int, SJ>{});
                            double colv[MD];
                            double gsb = gs[SJ];
                            double m   = pbest;
                            auto pick_rows = [&](auto qq) __attribute__((always_inline)) {
                                constexpr int q = decltype(qq)::value;
#pragma unroll
                                for (int r = cen; r < MD; r++)
                                    if ((r - cen) % 4 == q)
                                    {
                                        colv[r] = blk[SJ][r];
#pragma unroll
                                        for (int s = SJ + 1; s < NS; s++) colv[r] = sel(nxt_lbs == s, blk[s][r], colv[r]);
                                    }
                            };
                            m = dpp_max<0xB1>(m);
                            pick_rows(std::integral_constant<int, 0>{});
                            m = dpp_max<0x4E>(m);
                            pick_rows(std::integral_constant<int, 1>{});
                            m = dpp_max<0x141>(m);
                            pick_rows(std::integral_constant<int, 2>{});
                            m = dpp_max<0x140>(m);
                            pick_rows(std::integral_constant<int, 3>{});
#pragma unroll
                            for (int s = SJ + 1; s < NS; s++) gsb = sel(nxt_lbs == s, gs[s], gsb);
#pragma unroll
                            for (int r = (cen > j + 1 ? cen : j + 1); r < MD; r++) colv[r] = dfma(gsb, col[r], colv[r]);
#pragma unroll
                            for (int r = cen; r < MD; r += 2) D2(o_stage + gl * kHandoffStride + 8 * r) = qt_d2{colv[r], colv[r + 1]};
                            decide_finish(m);
                            fetch_column(std::integral_constant<int, j + 1>{}, nxt_w);
                        }
                        CSTAMP(5, (int)nxt_w)
                        // rows below of every live column
                        if constexpr (!(j + 1 < MD && SLJ == 1))
                        {
#pragma unroll
                            for (int s = SJ; s < NS; s++)
                            {
#pragma unroll
                                for (int r = j + 1; r < MD; r++) blk[s][r] = dfma(gs[s], col[r], blk[s][r]);
                            }
                        }
                        cur_lbs = nxt_lbs, cur_ispl = nxt_ispl, cur_w = nxt_w;
                        if constexpr (RET && j == 0)
                        {
                            // Slot S0 retires (see RETIRE).  Per problem, where step 0 made a pivot (cont; a problem that stopped keeps its
                            // registers as they are: nothing of its block is read again, and the level end stores its maps as before):
                            QT_MARK1("hh-retire", S0)
                            const int x0  = (int)(w0 & 15u);        // the pivot's lane and slot (uniform inside the problem)
                            const int ws0 = (int)((w0 >> 4) & 3u);
                            // (a) the pivot's place is finished: what the level end stores of it — row 0 of the image at the level's index 0, its
                            //     index byte, its physical column at position Fc — is stored now, by its lane
                            {
                                double w00 = blk[S0][0];
                                int wpc    = pc[S0];
#pragma unroll
                                for (int s = S0 + 1; s < NS; s++)
                                {
                                    w00 = sel(ws0 == s, blk[s][0], w00);
                                    wpc = sel(ws0 == s, pc[s], wpc);
                                }
                                if (cont && ispl0)
                                {
                                    D(o_img + 8 * imgoff)     = w00;
                                    B8(o_emap + 8 * wpc + k)  = (uint8_t)0;
                                    B8(o_phys + L.Fc)         = (uint8_t)wpc;
                                }
                            }
                            // (b) the pivot sits in an upper slot: the lone column (slot S0, lane 15) moves into its place — block, norm, position,
                            //     physical column — through the 8 MD + 16 bytes behind the sixteen hand-off slots
                            const int o_mv  = o_stage + 16 * kHandoffStride;
                            const bool mrow = cont && ws0 != S0;
                            if (mrow && gl == 15)
                            {
#pragma unroll
                                for (int r = 0; r < MD; r += 2) D2(o_mv + 8 * r) = qt_d2{blk[S0][r], blk[S0][r + 1]};
                                D2(o_mv + 8 * MD) = qt_d2{nrm[S0], __hiloint2double(pc[S0], pos[S0])};
                            }
                            quad_lds_fence();
                            double mc[MD];
#pragma unroll
                            for (int r = 0; r < MD; r += 2)
                            {
                                const qt_d2 v = D2(o_mv + 8 * r);
                                mc[r]         = v.x;
                                mc[r + 1]     = v.y;
                            }
                            const qt_d2 mt  = D2(o_mv + 8 * MD);
                            const bool recv = mrow && gl == x0;
#pragma unroll
                            for (int s = S0 + 1; s < NS; s++)
                            {
                                const bool hit = SL == 2 ? recv : (recv && ws0 == s);
#pragma unroll
                                for (int r = 0; r < MD; r++) blk[s][r] = sel(hit, mc[r], blk[s][r]);
                                nrm[s] = sel(hit, mt.x, nrm[s]);
                                pos[s] = sel(hit, __double2loint(mt.y), pos[s]);
                                pc[s]  = sel(hit, __double2hiint(mt.y), pc[s]);
                            }
                            // the decision for step 1 was made on the old places: where it chose the lone column, the pivot is now in lane x0
                            const bool lone1 = mrow && (int)((cur_w >> 4) & 3u) == S0;
                            cur_ispl         = lone1 ? gl == x0 : cur_ispl;
                            cur_lbs          = lone1 ? ws0 : cur_lbs;
                        }
                        CSTAMP(6, __double2loint(blk[NS - 1][MD - 1]))
                        FSTAMP(5)
                    });
                    if constexpr (RET) { QT_MARK1("hh-ret-end", S0) } else { QT_LMARK1("hh-end", S0) }
                    if (prefetch)
                        for_each_index<0, NH * NIH>([&](auto tt) __attribute__((always_inline)) {
                            if (decltype(tt)::value >= pf_issued) prefetch_piece(tt, F + dlev);
                        });
                    (void)SL;
                };

            // =====================================================================================
            // level end: triangular image [R_k T_k | rhs_k] / diag in end-of-level position order, maps
            // =====================================================================================
            // retired (RETIRE, wave-uniform): the level dropped slot kRetireSlot behind its first pivot step.  That slot's registers are stale where
            // the level made a pivot — its one live column was stored from the pivot's place or moved to it — and its store pass is skipped
            // there; a problem of rank 0 made no move and stores the slot's maps as ever
            auto level_end = [&](auto l0c, const int k, const qt_level &L, double (&blk)[NS][MD], const bool retired) __attribute__((always_inline)) {
                constexpr bool L0 = decltype(l0c)::value;
                (void)retired;
                const bool work = L.work;
                const int Fc = L.Fc, rank = L.rank;
                STAMP(5)
                LSTAMP(2)
                QT_LMARK("level-end")
                const int wk   = n + 1 - Fc;
                const int dump = o_stage + 8 * gl; // stores that do not apply go to a dump slot of the lane's own (the staging block is idle here): no divergent regions, no bank conflicts
                int roff[MD];          // byte offset of image row p (triangular packing), the same for every slot
#pragma unroll
                for (int p = 0; p < MD; p++) roff[p] = 8 * (p * wk - p * (p + 1) / 2);
#pragma unroll
                for (int s = 0; s < NS; s++)
                {
                    const int P0  = 16 * s + gl - SIG;
                    bool mv       = work && P0 <= n && P0 >= Fc; // columns that were live in this level (the RHS included)
                    if constexpr (RETIRE && !L0)
                    {
                        if (s == kRetireSlot) mv = mv && !(retired && rank > 0);
                    }
                    const int e   = pos[s] - Fc;                 // index of this column in the level's image: end-of-level position order
                    const int lim = mv ? (e < rank - 1 ? e : rank - 1) : -1; // rows 0 .. lim of the column go to the image (p < rank, p <= e)
                    const int base = o_img + 8 * (imgoff + e);
                    if (mv)
                    {
                        QT_LMARK1("level-end-store", s)
#pragma unroll
                        for (int p = 0; p < MD; p++) D(sel(p <= lim, base + roff[p], dump)) = blk[s][p];
                        B8(o_emap + 8 * pc[s] + k) = (uint8_t)e;
                        if (P0 < n) B8(o_phys + pos[s]) = (uint8_t)pc[s];
                    }
                    QT_LMARK1("level-end-maps", s)
                    // pivot position P0 of this level: its image row and the selector of this level's index byte
                    const bool piv = work && P0 >= Fc && P0 < Fc + rank;
                    const int p    = P0 - Fc;
                    rp[s]          = sel(piv, o_img + 8 * (imgoff + p * wk - p * (p + 1) / 2), rp[s]);
                    rq[s]          = sel(piv, 0x0c0c0c00 | k, rq[s]);
                }
                STAMP(6)
                LSTAMP(3)
                if (gl == 0)
                {
                    U32(o_meta + 16 * k)      = (uint32_t)Fc;
                    U32(o_meta + 16 * k + 4)  = (uint32_t)rank;
                    U32(o_meta + 16 * k + 8)  = (uint32_t)imgoff;
                    U32(o_meta + 16 * k + 12) = (uint32_t)wk;
                }
                quad_lds_fence();
                imgoff += wk * rank - rank * (rank - 1) / 2;
                TotalRank += rank;
            };

            // ---- level 0, peeled: its block is blk0 (requested at the top of the kernel); the layout is the identity, which is also what o_phys
            //      and o_emap hold (set above; the levels behind and the solve read them), so pos / pc / em come without look-ups; nothing is
            //      staged and nothing eliminated (no finished pivot: ColIndex == 0), every slot is live: factor_level<0>.  The next level's pieces
            //      are requested inside its pivot steps as inside any level's ----
            if constexpr (PEEL)
            {
                qt_level L;
                if (level_head(std::true_type{}, 0, L)) // (nObj >= 1: lexls_lse_create)
                {
#pragma unroll
                    for (int s = 0; s < NS; s++)
                    {
                        const int P = 16 * s + gl - SIG;
                        pc[s]       = (P >= 0 && P <= n) ? P : 0;
                        pos[s]      = (P >= 0 && P <= n) ? P : 0x3fffff;
                        em[s]       = 0ull;
                    }
                    level_post(std::true_type{}, 0, L, blk0);
                    { // (no elimination: its stamps read zero)
                        constexpr int k = 0;
                        (void)k;
                        STAMP(7)
                        LSTAMP(1)
                    }
                    factor_level(std::true_type{}, std::integral_constant<int, 0>{}, std::false_type{}, 0, L, blk0);
                    level_end(std::true_type{}, 0, L, blk0, false);
                }
            }
            // LDS order across the boundary, as between any two levels: the fence that ends level_end (behind the meta store) stands between
            // level 0's image / o_emap / o_phys / o_perm / meta stores and what the loop's first level reads — the o_phys / o_emap look-ups of
            // level_start, the image rows of the elimination — and between level 0's last hand-off reads of the staging block and the first staged
            // pieces written over it.  The fence behind the LDS set-up covers the o_phys / o_emap / o_xs initialisation for every later reader.
            // The s_nop that ends the elimination (DPP reads behind qt_gauss_dpp_self's writes) belongs to the loop's levels alone: level 0's
            // block is written by compiler-visible instructions only, whose hazards the compiler counts itself.

            // ---- the levels behind it.  The block is local to the iteration: level_start writes all of it (both row parts) before anything
            //      reads it, level_end reads it last — nothing of it crosses the back edge ----
            for (int k = PEEL ? 1 : 0; k < nObj; k++)
            {
                qt_level L;
                if (!level_head(std::false_type{}, k, L)) continue;
                double blk_k[NS][MD];                                // the level block, position layout
                double(&blk)[NS][MD] = *(PEEL ? &blk_k : &blk0);     // (the unpeeled shape: one block for all levels, carried round the loop)
                level_start(k, L, blk);
                level_post(std::false_type{}, k, L, blk);
                eliminate(k, L, blk);
                QT_MARK("hh-select")
                bool retired = false; // (wave-uniform)
                {
                    // (a rank-deficient level 0 leaves level 1 at column < 16 - SIG: all four choices stay)
                    const int fcmin = rows_min(L.work ? L.Fc : 0x3fffffff);
                    const int s0    = (fcmin + SIG) >> 4;
                    // (RETIRE) all four problems work and start the level at the same column, whose place is lane 15 of slot NS - 2: that slot
                    // holds one live column per problem (the right-hand side sits in the top slot)
                    if constexpr (RETIRE)
                        retired = __ballot(!L.work) == 0ull && rows_max(L.Fc) == fcmin && s0 == kRetireSlot && ((fcmin + SIG) & 15) == 15;
                    if (RETIRE && retired)
                        factor_level(std::false_type{}, std::integral_constant<int, (RETIRE ? kRetireSlot : 0)>{}, std::integral_constant<bool, RETIRE>{}, k, L, blk);
                    else if (NS > 3 && s0 >= 3)
                        factor_level(std::false_type{}, std::integral_constant<int, (NS > 3 ? 3 : 0)>{}, std::false_type{}, k, L, blk);
                    else if (NS > 2 && s0 >= 2)
                        factor_level(std::false_type{}, std::integral_constant<int, (NS > 2 ? 2 : 0)>{}, std::false_type{}, k, L, blk);
                    else if (NS > 1 && s0 >= 1)
                        factor_level(std::false_type{}, std::integral_constant<int, (NS > 1 ? 1 : 0)>{}, std::false_type{}, k, L, blk);
                    else
                        factor_level(std::false_type{}, std::integral_constant<int, 0>{}, std::false_type{}, k, L, blk);
                }
                level_end(std::false_type{}, k, L, blk, retired);
            }

            // ---- solve(): block back-substitution on the normalised images (lexlse.h:1015-1045); lane p <-> row p of a level.  Straight-line
            // per level: what does not apply reads a zero (position 16 NS - 1 of the x block is never written) or goes to the dump slot ----
            QT_MARK("solve-top")
            const int o_zero = o_xs + 8 * (16 * NS - 1);
            for (int k = nObj; k--;)
            {
                QT_MARK("solve-level")
                const qt_u4 mt = U4(o_meta + 16 * k); // {first column, rank, image offset, image width}
                const int rank = live ? (int)mt.y : 0;
                const int rmax = rows_max(rank);
                if (rmax == 0) continue;
                const int Fc = (int)mt.x, ok = (int)mt.z, wk = (int)mt.w;
                const int c0   = Fc + rank;
                const int acc  = rank > 0 ? TotalRank - c0 : 0;
                const int amax = rows_max(acc);
                const int p    = gl < rank ? gl : 0;
                const int row  = o_img + 8 * (ok + p * wk - p * (p + 1) / 2);
                double col[MD];
#pragma unroll
                for (int j = 1; j < MD; j++) col[j] = D(sel(j < rank && gl < j, row + 8 * j, o_zero));
                double sv = D(sel(gl < rank, row + 8 * (n - Fc), o_zero));
                // rhs'_k - T'_k x_later (lexlse.h:1029-1033): the column at final position c sits at its level-k index inside the image;
                // sixteen solved positions per trip — lane j looks up index and x of position c0 + base + j, the row-broadcast hands them out
                for (int base = 0; base < amax; base += 16)
                {
                    QT_MARK("solve-trip")
                    const bool have = base + gl < acc;
                    const int c     = have ? c0 + base + gl : 16 * NS - 1;
                    const int ph    = (int)B8(o_phys + c);
                    const int offv  = have ? (int)B8(o_emap + 8 * ph + k) : 0;
                    const double xv = D(o_xs + 8 * c); // (zero where the position does not apply)
                    double uj[16]; // all sixteen reads in flight before the first is used (issued a few at a time, each group pays the LDS latency)
                    for_each_index<0, 16>([&](auto jj) {
                        constexpr int j = decltype(jj)::value;
                        uj[j]           = D(row + 8 * gbci<j>(offv));
                    });
                    __builtin_amdgcn_sched_barrier(0);
                    double s0 = 0.0, s1 = 0.0; // two chains
                    for_each_index<0, 16>([&](auto jj) {
                        constexpr int j = decltype(jj)::value;
                        if (j & 1)
                            s1 = dfma(-uj[j], gbc<j>(xv), s1);
                        else
                            s0 = dfma(-uj[j], gbc<j>(xv), s0);
                    });
                    sv += s0 + s1;
                }
                QT_MARK("solve-tail")
                sv = sel(gl < rank, sv, 0.0);
                for_each_index<1, MD>([&](auto jj) {
                    constexpr int j = MD - decltype(jj)::value; // MD-1 .. 1
                    sv = dfma(-col[j], gbc<j>(sv), sv); // unit diagonal; col[j] is zero at and below the diagonal and beyond the rank
                });
                D(sel(gl < rank, o_xs + 8 * (Fc + gl), o_stage + 8 * gl)) = sv;
                quad_lds_fence();
            }
            STAMP(9)
            // ---- results ----
            QT_MARK("output")
            if (live)
            {
#pragma unroll
                for (int s = 0; s < NS; s++)
                {
                    const int P = 16 * s + gl; // every position once, whatever the layout offset
                    if (P < n)
                    {
                        a.x[(size_t)b * n + B8(o_phys + P)] = D(o_xs + 8 * P); // x = P x: the variable at position P (lexlse.h:1044)
                        a.perm[(size_t)b * n + P]           = (P < TotalRank) ? (uint32_t)B8(o_perm + P) : (uint32_t)P;
                    }
                }
                if (gl < nObj)
                {
                    a.fcol[(size_t)b * nObj + gl] = U32(o_meta + 16 * gl);
                    a.rank[(size_t)b * nObj + gl] = U32(o_meta + 16 * gl + 4);
                }
                if (gl == 0) a.totalrank[b] = (uint32_t)TotalRank;
            }
            if constexpr (EST)
            {
                const double e2 = row_max16(est2);
                if (gl == 0 && live) est_out[b] = e2 > 0.0 ? 2.0 * qt_sqrt(e2) : 0.0; // (no pivot at all: nothing to vouch for; a skipped problem keeps its estimate)
            }
            STAMP(10)
            STAMP_WRITE
#ifdef LEXLS_QTOL_CHAIN
            if (lane == 0)
                for (int i_ = 0; i_ < 7; i_++) a.lambda[(size_t)b * (n + cap) + 30 + i_] = (double)cacc[i_];
#endif

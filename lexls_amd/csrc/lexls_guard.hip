// The accuracy guard's compaction (lexls_lse_set_accuracy_guard): the estimates lqr_qtol's guarded instantiations wrote become a status per
// problem and, in mode 2, the list of problems the bit-exact kernel re-solves — in the stream, without the host.
//   status[b] = 1 when est[b] < threshold, else 2 (mode 1: reported) or 3 (mode 2: re-solved); a NaN estimate is flagged.
//   mode 2: ind[1 + i] = the i-th flagged problem (in no particular order), ind[0] = their number.  ind[0] starts at zero: the estimating
//   kernel in front of this one clears it.
// One wavefront's flags become one ballot; the flagged lanes take consecutive slots behind ONE atomic add on the counter per wavefront
// (by the wavefront's first flagged lane; the base goes to the others by a lane read).
#include "lexls_kernels.h"
#include "lexls_launch.h"

namespace lexls
{
    namespace
    {
        __global__ __launch_bounds__(256) void guard_compact_kernel(const double *est, uint8_t *status, uint32_t *ind, uint32_t batch, double threshold, int mode)
        {
            const uint32_t b    = blockIdx.x * 256u + threadIdx.x;
            const bool in_batch = b < batch;
            const double e      = in_batch ? est[b] : 0.0;
            const bool flagged  = in_batch && !(e < threshold);
            if (in_batch) status[b] = flagged ? (uint8_t)(mode == 2 ? 3 : 2) : (uint8_t)1;
            if (mode != 2) return;
            const unsigned long long m = __ballot(flagged);
            if (m == 0ull) return; // (wave-uniform)
            const int lane  = (int)(threadIdx.x & 63u);
            const int first = __ffsll((long long)m) - 1;
            const unsigned below = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u)); // flagged lanes below this one
            uint32_t base = 0;
            if (lane == first) base = atomicAdd(ind, (uint32_t)__popcll(m));
            base = (uint32_t)__builtin_amdgcn_readlane((int)base, first);
            if (flagged) ind[1 + base + below] = b;
        }

        /// a bit-exact kernel solved under a skip mask: status 0 and no estimate for the problems it solved, the report of a skipped problem kept
        __global__ __launch_bounds__(256) void guard_clear_kernel(double *est, uint8_t *status, const uint8_t *skip, uint32_t batch)
        {
            const uint32_t b = blockIdx.x * 256u + threadIdx.x;
            if (b < batch && !skip[b]) est[b] = 0.0, status[b] = (uint8_t)0;
        }
    } // namespace

    hipError_t launch_guard_clear(double *est, uint8_t *status, const uint8_t *skip, uint32_t batch, hipStream_t s)
    {
        hipLaunchKernelGGL(guard_clear_kernel, dim3((batch + 255u) / 256u), dim3(256), 0, s, est, status, skip, batch);
        return hipGetLastError();
    }

    hipError_t launch_guard_compact(const double *est, uint8_t *status, uint32_t *ind, uint32_t batch, double threshold, int mode, hipStream_t s)
    {
        hipLaunchKernelGGL(guard_compact_kernel, dim3((batch + 255u) / 256u), dim3(256), 0, s, est, status, ind, batch, threshold, mode);
        return hipGetLastError();
    }
} // namespace lexls

// The kernel table: every launcher of LEXLS_KERNEL_LIST (lexls_dispatch.h) behind one signature.  Each instantiation lives in its own
// translation unit (lqr_small_<shape>.hip, lqr_quad_*.hip, ...) so that they compile in parallel; which one serves a shape is plan_lqr's.
#include "lexls_kernels.h"
#include "lexls_launch.h"

#include <cstdlib>

namespace lexls
{
    // one launcher per kind of LEXLS_KERNEL_LIST entry: the instantiation's own launcher behind the table's signature.  Declared at block scope,
    // where it is called, on purpose: a signature that drifts from its instantiation macro (LEXLS_*_INSTANCE) fails at link time, as a forward declaration would
    using Launcher = hipError_t (*)(const LseArgs &, hipStream_t, const LaunchExtras &);
#define LEXLS_LAUNCH_NONE(fn) nullptr
#define LEXLS_LAUNCH_PLAIN(fn) [](const LseArgs &a, hipStream_t s, const LaunchExtras &) { hipError_t fn(const LseArgs &, hipStream_t); return fn(a, s); }
#define LEXLS_LAUNCH_EST(fn) [](const LseArgs &a, hipStream_t s, const LaunchExtras &x) { hipError_t fn(const LseArgs &, hipStream_t, double *, uint32_t *); return fn(a, s, x.est, x.ind); }
#define LEXLS_LAUNCH_IND(fn) [](const LseArgs &a, hipStream_t s, const LaunchExtras &x) { hipError_t fn(const LseArgs &, hipStream_t, const uint32_t *); return fn(a, s, x.ind); }
#define LEXLS_LAUNCH_REG(fn) [](const LseArgs &a, hipStream_t s, const LaunchExtras &x) { hipError_t fn(const LseArgs &, hipStream_t, uint32_t *); return fn(a, s, x.reg_cfg); }
#define LEXLS_LAUNCH_FUSED(fn)                                                                                                                  \
    [](const LseArgs &a, hipStream_t s, const LaunchExtras &x) {                                                                                \
        hipError_t fn(const LseArgs &, uint32_t, const int32_t *, double, double, bool, const void *, size_t, int, hipStream_t);                \
        const FusedCall &f = *x.fused;                                                                                                          \
        return fn(a, f.sweep_level_dim, f.d_obj_index, f.tolW, f.tolC, f.scan_up, f.resident_args, f.resident_args_bytes, f.count, s);         \
    }
    static const Launcher kLaunchers[] = {
#define LEXLS_X(id, name, kind, fn) LEXLS_LAUNCH_##kind(fn),
        LEXLS_KERNEL_LIST(LEXLS_X)
#undef LEXLS_X
    };

    hipError_t launch_kernel(KernelId id, const LseArgs &a, hipStream_t s, const LaunchExtras &x)
    {
        const Launcher l = kLaunchers[(int)id];
        return l ? l(a, s, x) : hipErrorNotSupported;
    }

    /// LDS one wavefront of a REG launch may fill with the regularization routines' optional pieces (work matrix, null-space basis): a CU's LDS
    /// over LEXLS_REG_LDS_WAVES (1 .. 8, default 8) wavefronts.  Read at the first call and kept for the life of the process.
    size_t wave_reg_lds_share()
    {
        static const size_t share = [] {
            const char *e = std::getenv("LEXLS_REG_LDS_WAVES");
            const long w  = e ? std::atol(e) : 8;
            return kMaxLdsBytes / (size_t)(w < 1 ? 1 : (w > 8 ? 8 : w));
        }();
        return share;
    }

    /// waves of the register-resident kernel the device holds at once (2 per SIMD): up to that many problems run in ONE round of it
    uint32_t resident_wave_capacity()
    {
        static uint32_t cap_of[64] = {0}; // per device (a process may drive several)
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256u * 4u * 2u;
        if (!cap_of[dev])
        {
            int cus = 0;
            if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
            cap_of[dev] = (uint32_t)cus * 4u * 2u;
        }
        return cap_of[dev];
    }
} // namespace lexls

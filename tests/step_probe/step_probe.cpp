// TEST INFRASTRUCTURE ONLY -- never part of the product build.
//
// Probe library for tests/test_newton_step.py: ONE iteration of the interior-point loop of scpp_amd/csrc/ipm_solve.h (ipmSolveInstance) and its
// once-per-solve start points, phase after phase in the order and with the early exits of that function's text, on record blocks the test has filled,
// so that the Newton system and the start-point problems they claim to solve can be solved again by a reference that shares nothing with them
// (tests/newton_reference.py).  No solver code, no copy of a function under test and no arithmetic of its own lives here.
//
// Built by hipcc for gfx950 with the product's flags, a second time with -DIPM_SPLIT_STEPS=0 (the compile-time common step length), and by g++ against
// the wave emulator (__graft_entry__.py).
// Geometry: the product's -- one 64-lane wavefront per block and instance, __shared__ Ctx, Glob, Iter and TileShared handed over by LDS address, dynamic
// LDS of segLdsBytes<P>(K); the guard item < count and every branch on the job description are wave-uniform.  Jobs of different models, modes, policies
// and horizons share one launch.
// Memory: ONE arena of doubles per launch, copied in, worked on, copied out; a job names EVERY block of a Ctx by offsets into it.  What lies between the
// blocks is the caller's (a sentinel pattern), and the caller sees every byte of it again.  Glob and Iter travel as flat arrays of doubles (the four
// ints of Iter as doubles), in the order of tests/phase_probe's phase_probe_glob_names / phase_probe_iter_names.
#include "../../scpp_amd/csrc/ipm_solve.h"

#include <cstddef>

namespace
{
using namespace scpp;
using namespace scpp::ipm;

enum Desc
{
    D_MODEL = 0, // 0 RocketQuatSC, 1 Rocket2dSC, 2 Lander3dofSC, 3 ZeroOrderHold<RocketQuatSC>
    D_POLICY,    // 0: nu, nu_b, lam live in LDS ; 1: SegFieldsInWorkspace<...>
    D_K,
    D_OP,        // enum Op
    D_SETUP_V0,  // Ctx::setup_v0 (OP_WARM: the element-wise form of the warm start)
    DESC_N
};
enum Op
{
    OP_ITER = 0,   // the chain of one iteration up to the corrector's direction
    OP_ITER_STEP,  // ... then phUpdate
    OP_ITER_FUSED, // ... then phResiduals<P, true>
    OP_PREDICT,    // the chain up to and including phDirSeg<0>
    OP_COLD,       // the cold start (ECOS init, W = I) on records as phSetup leaves them
    OP_WARM,       // solveWarmInit
    OP_N
};
enum Offs
{
    O_SX = 0, // [K][XREC]
    O_ST,     // [STREC][pitch]
    O_SG,     // [G_NFIELDS * NL][pitch]
    O_DY,     // [DYNREC][pitch]
    O_FAC,    // [K][FACREC]
    O_SV,     // [K][SVREC]
    O_GSAVE,  // [GSAVE]
    O_A,      // [K - 1][NX][NX]
    O_B,      // [K - 1][NX][NU]
    O_C,      // [K - 1][NX][NU]
    O_S,      // [K - 1][NX]
    O_Z,      // [K - 1][NX]
    O_IP,     // [IP_N]
    O_GLOB,   // [GLOB_N]
    O_ITER,   // [ITER_N]
    OFF_N
};

constexpr int GLOB_N = int(sizeof(Glob) / sizeof(double));
constexpr int ITER_D = int(offsetof(Iter, D) / sizeof(double));
constexpr int ITER_N = ITER_D + 4;
static_assert(sizeof(Glob) == GLOB_N * sizeof(double) && GLOB_N == 44, "the flat order of Glob is phase_probe_glob_names");
static_assert(offsetof(Iter, D) == ITER_D * sizeof(double) && ITER_D == 41, "the flat order of Iter is phase_probe_iter_names");

// the text of ipmSolveInstance, one iteration (or one start point) of it
template <class P>
__device__ inline void runOp(const LDSP Ctx *cs, LDSP Glob *gp, LDSP Iter *itp, TileShared &sh, int op, bool scvx)
{
    if (op == OP_COLD)
    {
        phInitPrimalRhs<P>(cs, gp, itp);
        {
            const RhsSpec sp = specBorderPlus();
            factorSweepAny<P>(cs, sh, sp);
            bwdSweepAny<P>(cs, sp);
        }
        phInitPrimalFinish<P>(cs, gp, itp);
        phInitDualRhs<P>(cs, gp, itp);
        {
            const RhsSpec sp = specSingle();
            fwdSweepAny<P>(cs, sp);
            bwdSweepAny<P>(cs, sp);
        }
        phInitDualFinish<P>(cs, gp, itp);
        return;
    }
    if (op == OP_WARM)
    {
        solveWarmInit<P>(cs, gp, itp);
        return;
    }
    phSegLdsCopy<P, true>(cs);
    phResiduals<P, false>(cs, gp, itp);
    phScalings<P>(cs, gp, itp);
    if (!uniformInt(itp->bad))
    {
        phRhs<P, 0>(cs, gp, itp);
        {
            const RhsSpec sp = scvx ? specSingle() : specBorderPlus();
            factorSweepAny<P>(cs, sh, sp);
            bwdSweepAny<P>(cs, sp);
        }
        phDirStage<P, 0>(cs, gp, itp);
        phDirSeg<P, 0>(cs, gp, itp);
        if (op != OP_PREDICT && !uniformInt(itp->bad))
        {
            phRhs<P, 1>(cs, gp, itp);
            {
                const RhsSpec sp = specSingle();
                fwdSweepAny<P>(cs, sp);
                bwdSweepAny<P>(cs, sp);
            }
            phDirStage<P, 1>(cs, gp, itp);
            phDirSeg<P, 1>(cs, gp, itp);
            if (!uniformInt(itp->bad))
            {
                if (op == OP_ITER_STEP)
                    phUpdate<P>(cs, gp, itp);
                else if (op == OP_ITER_FUSED)
                    phResiduals<P, true>(cs, gp, itp);
            }
        }
    }
    phSegLdsCopy<P, false>(cs);
}
template <class P>
__device__ inline void runPolicy(const LDSP Ctx *cs, LDSP Glob *gp, LDSP Iter *itp, TileShared &sh, int policy, int op, bool scvx)
{
    if (policy == 0)
        runOp<P>(cs, gp, itp, sh, op, scvx);
    else
        runOp<SegFieldsInWorkspace<P>>(cs, gp, itp, sh, op, scvx);
}

// (2: the product's IPM_WAVES_PER_SIMD, ipm_solve.h)
__global__ void __launch_bounds__(WAVE, 2) __attribute__((disable_tail_calls)) step_kernel(int count, const int *desc, const long long *offs, double *arena)
{
    const int item = blockIdx.x;
    if (item >= count)
        return;
    const int lane = threadIdx.x;
    const int *d = desc + item * DESC_N;
    const long long *o = offs + item * OFF_N;
    const int model = uniformInt(d[D_MODEL]), policy = uniformInt(d[D_POLICY]), op = uniformInt(d[D_OP]);
    __shared__ TileShared sh;
    __shared__ Ctx cshared;
    __shared__ Glob gshared;
    __shared__ Iter itshared;
#ifdef SCPP_HIP_EMU
    static double seg_lds[NSEGLDS * 16 * 64];
    LDSP double *segl = seg_lds;
#else
    extern __shared__ __attribute__((aligned(16))) double seg_lds[];
    LDSP double *segl = (LDSP double *)seg_lds;
#endif
    Ctx c;
    c.segl = segl;
    c.K = uniformInt(d[D_K]);
    c.lane = lane;
    c.pitch = recPitch(c.K);
    c.setup_v0 = uniformInt(d[D_SETUP_V0]);
    c.sx = arena + o[O_SX];
    c.st = arena + o[O_ST];
    c.sg = arena + o[O_SG];
    c.dy = arena + o[O_DY];
    c.fac = arena + o[O_FAC];
    c.sv = arena + o[O_SV];
    c.gsave = arena + o[O_GSAVE];
    c.A = arena + o[O_A];
    c.B = arena + o[O_B];
    c.C = arena + o[O_C];
    c.S = arena + o[O_S];
    c.Z = arena + o[O_Z];
    c.ip = arena + o[O_IP];
    const bool scvx = uniformInt(int(c.ip[IP_SCVX] != 0.)) != 0;
    double *gflat = arena + o[O_GLOB], *iflat = arena + o[O_ITER];
    const LDSP Ctx *cs = (const LDSP Ctx *)&cshared;
    LDSP Glob *gp = (LDSP Glob *)&gshared;
    LDSP Iter *itp = (LDSP Iter *)&itshared;
    if (lane == 0)
    {
        cshared = c;
        LDSP double *gd = (LDSP double *)gp, *id = (LDSP double *)itp;
        for (int i = 0; i < GLOB_N; i++)
            gd[i] = gflat[i];
        for (int i = 0; i < ITER_D; i++)
            id[i] = iflat[i];
        itp->D = int(iflat[ITER_D]);
        itp->bad = int(iflat[ITER_D + 1]);
        itp->bk_valid = int(iflat[ITER_D + 2]);
        itp->common_step = int(iflat[ITER_D + 3]);
    }
    WAVE_SYNC();
    switch (model)
    {
    case 0: runPolicy<RocketQuatSC>(cs, gp, itp, sh, policy, op, scvx); break;
    case 1: runPolicy<Rocket2dSC>(cs, gp, itp, sh, policy, op, scvx); break;
    case 2: runPolicy<Lander3dofSC>(cs, gp, itp, sh, policy, op, scvx); break;
    case 3: runPolicy<ZeroOrderHold<RocketQuatSC>>(cs, gp, itp, sh, policy, op, scvx); break;
    default: break;
    }
    WAVE_SYNC();
    if (lane == 0)
    {
        const LDSP double *gd = (const LDSP double *)gp, *id = (const LDSP double *)itp;
        for (int i = 0; i < GLOB_N; i++)
            gflat[i] = gd[i];
        for (int i = 0; i < ITER_D; i++)
            iflat[i] = id[i];
        iflat[ITER_D] = double(itp->D);
        iflat[ITER_D + 1] = double(itp->bad);
        iflat[ITER_D + 2] = double(itp->bk_valid);
        iflat[ITER_D + 3] = double(itp->common_step);
    }
}

template <class F>
bool withModel(int model, F &&f)
{
    switch (model)
    {
    case 0: f(RocketQuatSC{}); return true;
    case 1: f(Rocket2dSC{}); return true;
    case 2: f(Lander3dofSC{}); return true;
    case 3: f(ZeroOrderHold<RocketQuatSC>{}); return true;
    default: return false;
    }
}

// doubles of every block of a job: interface constants, no arithmetic of the solver's
bool blockSizes(int model, int K, long long *need)
{
    return withModel(model, [&](auto p) {
        using P = decltype(p);
        using L = Lay<P>;
        const long long pitch = recPitch(K), k1 = K - 1;
        need[O_SX] = (long long)K * L::XREC;
        need[O_ST] = L::STREC * pitch;
        need[O_SG] = (long long)G_NFIELDS * L::NL * pitch;
        need[O_DY] = L::DYNREC * pitch;
        need[O_FAC] = (long long)K * L::FACREC;
        need[O_SV] = (long long)K * SVREC;
        need[O_GSAVE] = GSAVE;
        need[O_A] = k1 * P::NX * P::NX;
        need[O_B] = need[O_C] = k1 * P::NX * P::NU;
        need[O_S] = need[O_Z] = k1 * P::NX;
        need[O_IP] = IP_N;
        need[O_GLOB] = GLOB_N;
        need[O_ITER] = ITER_N;
    });
}

struct Dev
{
    void *p = nullptr;
    int err = 0;
    Dev(const void *host, size_t bytes)
    {
        if (hipMalloc(&p, bytes ? bytes : 8) != hipSuccess)
            err = 1;
        else if (bytes && host && hipMemcpy(p, host, bytes, hipMemcpyHostToDevice) != hipSuccess)
            err = 1;
    }
    ~Dev()
    {
        if (p)
            (void)hipFree(p);
    }
};

} // namespace

extern "C"
{

int step_probe_split_steps() { return IPM_SPLIT_STEPS; }
int step_probe_off_n() { return OFF_N; }
int step_probe_desc_n() { return DESC_N; }
// the blocks of a job in the order of its offsets, and the ops in the order of enum Op
const char *step_probe_block_names() { return "sx st sg dy fac sv gsave A B C S Z ip glob iter"; }
const char *step_probe_op_names() { return "ITER ITER_STEP ITER_FUSED PREDICT COLD WARM"; }
// need[OFF_N]: the doubles of every block of a job.  0; 3: an unknown model or a horizon the phases do not admit
int step_probe_block_sizes(int model, int K, long long *need)
{
    if (K < 3 || K > 64)
        return 3;
    return blockSizes(model, K, need) ? 0 : 3;
}
// the flat positions of the Hessian outputs a caller cannot get from the other probes' layouts: out = {X_HS, X_HC, HS_N, FACREC, SVREC, GSAVE, F_ETA, F_WB}
int step_probe_extra_layout(int model, int *out)
{
    return withModel(model, [&](auto p) {
        using L = Lay<decltype(p)>;
        out[0] = L::X_HS, out[1] = L::X_HC, out[2] = L::HS_N, out[3] = L::FACREC, out[4] = SVREC, out[5] = GSAVE, out[6] = L::F_ETA, out[7] = L::F_WB;
    }) ? 0 : 3;
}

// Runs `count` jobs in ONE launch on the arena (copied to the device, copied back whole).  0; 1: the runtime reported an error; 2: a bad count;
// 3: a job description the phases do not admit; 4: a block that does not lie inside the arena or is not aligned as the product aligns it (nothing is
// launched then)
int step_probe_run(int count, const int *desc, const long long *offs, double *arena, long long arena_doubles)
{
    if (count <= 0 || arena_doubles <= 0)
        return 2;
    unsigned lds = 0;
    for (int q = 0; q < count; q++)
    {
        const int *d = desc + q * DESC_N;
        const long long *o = offs + q * OFF_N;
        long long need[OFF_N];
        if (d[D_K] < 3 || d[D_K] > 64 || d[D_POLICY] < 0 || d[D_POLICY] > 1 || d[D_OP] < 0 || d[D_OP] >= OP_N || d[D_SETUP_V0] < 0 || d[D_SETUP_V0] > 1 ||
            !blockSizes(d[D_MODEL], d[D_K], need))
            return 3;
        withModel(d[D_MODEL], [&](auto p) {
            const unsigned b = d[D_POLICY] == 0 ? segLdsBytes<decltype(p)>(d[D_K]) : 0u;
            lds = b > lds ? b : lds;
        });
        for (int f = 0; f < OFF_N; f++)
        {
            if (o[f] < 0 || o[f] > arena_doubles || need[f] > arena_doubles - o[f])
                return 4;
            // the record blocks and the factor block start on a 128-byte line in the product's workspace; the pitch keeps rows 16-byte aligned
            if ((f == O_SX || f == O_FAC || f == O_SV) ? (o[f] % 16 != 0) : (f <= O_DY && o[f] % 2 != 0))
                return 4;
        }
    }
    const size_t bytes = size_t(arena_doubles) * 8;
    Dev ddesc(desc, size_t(count) * DESC_N * sizeof(int)), doffs(offs, size_t(count) * OFF_N * sizeof(long long)), darena(arena, bytes);
    if (ddesc.err || doffs.err || darena.err)
        return 1;
    hipLaunchKernelGGL(step_kernel, dim3(count), dim3(WAVE), lds, nullptr, count, static_cast<const int *>(ddesc.p), static_cast<const long long *>(doffs.p),
                       static_cast<double *>(darena.p));
    const int e1 = hipGetLastError() != hipSuccess, e2 = hipDeviceSynchronize() != hipSuccess;
    if (e1 || e2)
        return 1;
    return hipMemcpy(arena, darena.p, bytes, hipMemcpyDeviceToHost) != hipSuccess ? 1 : 0;
}

} // extern "C"

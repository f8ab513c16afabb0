// TEST INFRASTRUCTURE ONLY -- never part of the product build.
//
// Probe library for tests/test_sweeps.py: one kernel that runs the factor, forward and backward sweeps of scpp_amd/csrc/sweeps.h ALONE,
// on record blocks the test has filled, so that the linear system they claim to solve can be solved again by a reference that shares
// nothing with them (tests/sweep_reference.py).  No solver code and no copy of a function under test lives here.
//
// Built twice (__graft_entry__.py): by hipcc for gfx950 with the product's flags, and by g++ against the wave emulator.
// Geometry: the product's (ipm_solve.h, ipm_split.h: ipm_factor_kernel) -- one 64-lane wavefront per block, one block per system, a
// __shared__ TileShared and a __shared__ Ctx written by lane 0 and handed to the sweeps by LDS address; the guard item < count and every
// branch on the job description are wave-uniform.  Systems of different models, horizons and column counts share one launch.
// Memory: ONE arena of doubles per launch, copied in, worked on, copied out; a job names its record blocks by offsets into it.  What lies
// between the blocks is the caller's (a sentinel pattern), and the caller sees every byte of it again.
#include "../../scpp_amd/csrc/sweeps.h"

namespace
{
using namespace scpp;
using namespace scpp::ipm;

// job description: desc[item][DESC_N] ints, offs[item][OFF_N] offsets (doubles) into the arena
enum Desc
{
    D_MODEL = 0, // 0 RocketQuatSC, 1 Rocket2dSC, 2 Lander3dofSC, 3 ZeroOrderHold<RocketQuatSC>
    D_K,
    D_N,    // RhsSpec.n
    D_OP,   // 0 factor (factor sweep with its fused forward pass, backward sweep), 1 resolve (forward sweep, backward sweep)
    D_FORM, // 0 what the product selects (*SweepAny), 1 the tile form (factorSweepFused<P, 0>, fwdSweep, bwdSweep)
    DESC_N
};
enum Offs
{
    O_SX = 0,
    O_FAC,
    O_SV,
    O_A,
    O_B,
    O_C,
    O_IP,
    O_UNUSED, // st, sg, dy, gsave, S, Z: not used by the sweeps; they point at a small block of the caller's
    OFF_N
};
constexpr int UNUSED_DOUBLES = 16;
constexpr int NMODELS = 4;

template <class P>
__device__ inline void runSweeps(const LDSP Ctx *cs, TileShared &sh, int n, int op, int form)
{
    RhsSpec sp;
    sp.n = n;
    if (form == 0)
    {
        if (op == 0)
            factorSweepAny<P>(cs, sh, sp);
        else
            fwdSweepAny<P>(cs, sp);
        bwdSweepAny<P>(cs, sp);
    }
    else
    {
        if (op == 0)
            factorSweepFused<P, 0>(cs, sh, sp);
        else
            fwdSweep<P>(cs, sp);
        bwdSweep<P>(cs, sp);
    }
}

// (2: the product's IPM_WAVES_PER_SIMD, ipm_solve.h)
__global__ void __launch_bounds__(WAVE, 2) __attribute__((disable_tail_calls)) sweep_kernel(int count, const int *desc, const long long *offs, double *arena)
{
    const int item = blockIdx.x;
    if (item >= count)
        return;
    const int lane = threadIdx.x;
    const int *d = desc + item * DESC_N;
    const long long *o = offs + item * OFF_N;
    const int model = uniformInt(d[D_MODEL]), n = uniformInt(d[D_N]), op = uniformInt(d[D_OP]), form = uniformInt(d[D_FORM]);
    __shared__ TileShared sh;
    __shared__ Ctx cshared;
    __shared__ double seglDummy[2];
    Ctx c;
    c.segl = (LDSP double *)seglDummy;
    c.K = uniformInt(d[D_K]);
    c.lane = lane;
    c.pitch = recPitch(c.K);
    c.sx = arena + o[O_SX];
    c.fac = arena + o[O_FAC];
    c.sv = arena + o[O_SV];
    c.A = arena + o[O_A];
    c.B = arena + o[O_B];
    c.C = arena + o[O_C];
    c.ip = arena + o[O_IP];
    c.st = c.sg = c.dy = c.gsave = arena + o[O_UNUSED];
    c.S = c.Z = arena + o[O_UNUSED];
    const LDSP Ctx *cs = (const LDSP Ctx *)&cshared;
    if (lane == 0)
        cshared = c;
    WAVE_SYNC();
    switch (model)
    {
    case 0: runSweeps<RocketQuatSC>(cs, sh, n, op, form); break;
    case 1: runSweeps<Rocket2dSC>(cs, sh, n, op, form); break;
    case 2: runSweeps<Lander3dofSC>(cs, sh, n, op, form); break;
    case 3: runSweeps<ZeroOrderHold<RocketQuatSC>>(cs, sh, n, op, form); break;
    default: break;
    }
}

// ---- what a caller of the sweeps must know about a model's records: interface constants, no arithmetic ----
enum LayoutField
{
    LF_NL = 0,
    LF_NVU,
    LF_NXV,
    LF_NUV,
    LF_NX,
    LF_NU,
    LF_XREC,
    LF_FACREC,
    LF_SVREC,
    LF_X_BETA,
    LF_X_BCW,
    LF_X_VW,
    LF_X_HS,
    LF_X_HC,
    LF_X_WBT,
    LF_X_RHO,
    LF_X_BCL,
    LF_X_VL,
    LF_X_EINV,
    LF_X_S,
    LF_FAC_LI,
    LF_FAC_YT,
    LF_FAC_TI,
    LF_HS_N,
    LF_IP_SCVX,
    LF_IP_N,
    LF_NRHS_MAX,
    LF_PAT,                // [16][16] Derived<P>::PAT.idx
    LF_XMAP = LF_PAT + 256, // [16], -1 beyond NXV
    LF_UMAP = LF_XMAP + 16, // [16], -1 beyond NUV
    LF_COUNT = LF_UMAP + 16
};
template <class P>
void fillLayout(int *out)
{
    using L = Lay<P>;
    out[LF_NL] = L::NL;
    out[LF_NVU] = L::NVU;
    out[LF_NXV] = P::NXV;
    out[LF_NUV] = P::NUV;
    out[LF_NX] = P::NX;
    out[LF_NU] = P::NU;
    out[LF_XREC] = L::XREC;
    out[LF_FACREC] = L::FACREC;
    out[LF_SVREC] = SVREC;
    out[LF_X_BETA] = L::X_BETA;
    out[LF_X_BCW] = L::X_BCW;
    out[LF_X_VW] = L::X_VW;
    out[LF_X_HS] = L::X_HS;
    out[LF_X_HC] = L::X_HC;
    out[LF_X_WBT] = L::X_WBT;
    out[LF_X_RHO] = L::X_RHO;
    out[LF_X_BCL] = L::X_BCL;
    out[LF_X_VL] = L::X_VL;
    out[LF_X_EINV] = L::X_EINV;
    out[LF_X_S] = L::X_S;
    out[LF_FAC_LI] = L::FAC_LI;
    out[LF_FAC_YT] = L::FAC_YT;
    out[LF_FAC_TI] = L::FAC_TI;
    out[LF_HS_N] = L::HS_N;
    out[LF_IP_SCVX] = IP_SCVX;
    out[LF_IP_N] = IP_N;
    out[LF_NRHS_MAX] = NRHS_MAX;
    for (int a = 0; a < NV; a++)
        for (int b = 0; b < NV; b++)
            out[LF_PAT + a * NV + b] = L::PAT.idx[a][b];
    for (int j = 0; j < 16; j++)
    {
        out[LF_XMAP + j] = j < P::NXV ? P::XMAP[j] : -1;
        out[LF_UMAP + j] = j < P::NUV ? P::UMAP[j] : -1;
    }
}
bool layoutOf(int model, int *out)
{
    switch (model)
    {
    case 0: fillLayout<RocketQuatSC>(out); return true;
    case 1: fillLayout<Rocket2dSC>(out); return true;
    case 2: fillLayout<Lander3dofSC>(out); return true;
    case 3: fillLayout<ZeroOrderHold<RocketQuatSC>>(out); return true;
    default: return false;
    }
}

struct Dev
{
    void *p = nullptr;
    int err = 0;
    Dev(const void *host, size_t bytes)
    {
        if (hipMalloc(&p, bytes ? bytes : 8) != hipSuccess)
            err = 1;
        else if (bytes && hipMemcpy(p, host, bytes, hipMemcpyHostToDevice) != hipSuccess)
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

int sweep_probe_layout_count() { return LF_COUNT; }

// names of the scalar fields of the layout, in the order of enum LayoutField; PAT [16][16], XMAP [16] and UMAP [16] follow them
const char *sweep_probe_layout_names()
{
    return "NL NVU NXV NUV NX NU XREC FACREC SVREC X_BETA X_BCW X_VW X_HS X_HC X_WBT X_RHO X_BCL X_VL X_EINV X_S FAC_LI FAC_YT FAC_TI HS_N IP_SCVX IP_N NRHS_MAX";
}

// out[LF_COUNT] (the order of enum LayoutField); 0, or 3 for an unknown model
int sweep_probe_layout(int model, int *out) { return layoutOf(model, out) ? 0 : 3; }

// Lay<P>::fixedMask(k, K), -1 for an unknown model
int sweep_probe_fixed_mask(int model, int k, int K)
{
    switch (model)
    {
    case 0: return int(Lay<RocketQuatSC>::fixedMask(k, K));
    case 1: return int(Lay<Rocket2dSC>::fixedMask(k, K));
    case 2: return int(Lay<Lander3dofSC>::fixedMask(k, K));
    case 3: return int(Lay<ZeroOrderHold<RocketQuatSC>>::fixedMask(k, K));
    default: return -1;
    }
}

// Runs `count` jobs in ONE launch on the arena (copied to the device, copied back whole).  0; 1: the runtime reported an error; 2: a bad count;
// 3: a job description the sweeps do not admit; 4: a record block that does not lie inside the arena (nothing is launched then)
int sweep_probe_run(int count, const int *desc, const long long *offs, double *arena, long long arena_doubles)
{
    if (count <= 0 || arena_doubles <= 0)
        return 2;
    for (int q = 0; q < count; q++)
    {
        const int *d = desc + q * DESC_N;
        const long long *o = offs + q * OFF_N;
        int lay[LF_COUNT];
        if (!layoutOf(d[D_MODEL], lay) || d[D_K] < 3 || d[D_K] > 64 || d[D_N] < 1 || d[D_N] > 2 || d[D_OP] < 0 || d[D_OP] > 1 || d[D_FORM] < 0 || d[D_FORM] > 1)
            return 3;
        const long long K = d[D_K];
        const long long need[OFF_N] = {K * lay[LF_XREC], K * lay[LF_FACREC], K * lay[LF_SVREC], (K - 1) * lay[LF_NX] * lay[LF_NX],
                                       (K - 1) * lay[LF_NX] * lay[LF_NU], (K - 1) * lay[LF_NX] * lay[LF_NU], lay[LF_IP_N], UNUSED_DOUBLES};
        for (int f = 0; f < OFF_N; f++)
            if (o[f] < 0 || o[f] > arena_doubles || need[f] > arena_doubles - o[f])
                return 4;
    }
    const size_t bytes = size_t(arena_doubles) * 8;
    Dev ddesc(desc, size_t(count) * DESC_N * sizeof(int)), doffs(offs, size_t(count) * OFF_N * sizeof(long long)), darena(arena, bytes);
    if (ddesc.err || doffs.err || darena.err)
        return 1;
    hipLaunchKernelGGL(sweep_kernel, dim3(count), dim3(WAVE), 0, nullptr, count, static_cast<const int *>(ddesc.p), static_cast<const long long *>(doffs.p),
                       static_cast<double *>(darena.p));
    const int e1 = hipGetLastError() != hipSuccess, e2 = hipDeviceSynchronize() != hipSuccess;
    if (e1 || e2)
        return 1;
    return hipMemcpy(arena, darena.p, bytes, hipMemcpyDeviceToHost) != hipSuccess ? 1 : 0;
}

} // extern "C"

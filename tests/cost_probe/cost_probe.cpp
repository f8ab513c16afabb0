// TEST INFRASTRUCTURE ONLY -- never part of the product build.
//
// Probe library for tests/test_cost_step.py: the SCvx cost step of scpp_amd/csrc/scvx_kernels.h ALONE.
//   * cost kernel, form 0: scvxCostUpdate<Model> (the pool engine's scvx_cost_update_kernel: one lane per segment), one wavefront per block, under
//     __launch_bounds__(WAVE, COST_WAVES_PER_SIMD) as the product has it;
//   * cost kernel, form 1: scvxCostUpdateSplit<Model> (what the persistent kernel runs: two lanes per segment, passes of 32 pairs) under
//     __launch_bounds__(WAVE, IPM_WAVES_PER_SIMD), the register budget it was written for; `seg_sum` is 64 doubles of LDS of the probe's, copied from and
//     to a block of the arena around the call, so that a test sees every segment's defect alone;
//   * decide kernel: one lane per case calls scvxDecide(b, v, so, i, nonlinear_cost) with a cost the test supplies;
//   * scvx_record_initial_kernel as the product launches it (one wavefront per instance, a second block beyond B).
// The cost kernels are templates over the model, as the product's are: every model keeps the registers its own flow map needs.
// No arithmetic and no copy of a function under test lives here.
//
// Built by hipcc for gfx950 with the product's flags and by g++ against the wave emulator (__graft_entry__.py).
// Memory: every array of SCBuffers / SCvxBuffers the step touches is a slice of ONE arena of doubles per launch, copied in, worked on, copied out; a job
// names its blocks by offsets into it.  What lies between the blocks is the caller's (a sentinel pattern), and the caller sees every byte of it again.
// The int fields travel as ints[job][INT_N] beside it.  Arrays the step has no business with point at a small block of the caller's (O_UNUSED, I_IPM_ITERS).
// A job is ONE instance (i = 0) of a batch of D_B instances: D_B = 1, or 0 for the guard i >= B.
#include "../../scpp_amd/csrc/ipm_solve.h"
#include "../../scpp_amd/csrc/scvx_kernels.h"

#include <cstddef>

namespace
{
using namespace scpp;
using namespace scpp::ipm;

enum Desc
{
    D_MODEL = 0, // 0 RocketQuatModel, 1 Rocket2dModel, 2 Lander3dofModel (the ABI's model ids)
    D_K,
    D_FORM,     // 0 scvxCostUpdate, 1 scvxCostUpdateSplit
    D_B,        // SCBuffers::B: 1, or 0 (the instance lies beyond the batch)
    D_ITER_CAP, // SCvxBuffers::iter_cap
    D_RING,     // 0: SCvxBuffers::iter_ring is null
    DESC_N
};
enum Offs
{
    O_X = 0,  // [K][NX]
    O_U,      // [K][NU]
    O_SIGMA,  // [1]
    O_IP,     // [IP_N]
    O_NU1,    // [1] norm1_nu
    O_XOLD,   // [K][NX]
    O_UOLD,   // [K][NU]
    O_TR,     // [1]
    O_LAST,   // [1]
    O_COST,   // [1]
    O_INFO,   // [4]
    O_RING,   // [iter_cap][K (NX + NU) + SCVX_ITER_SCALARS]
    O_SEG,    // [WAVE] seg_sum of form 1 (copied into LDS before the call and back after it)
    O_UNUSED, // x_init_dim, uhat, wtrx, sum_delta, delta_sigma: not used by this step
    OFF_N
};
enum Ints
{
    I_ACTIVE = 0,
    I_CONVERGED,
    I_SC_ITERS,
    I_IPM_ITERS, // not used by this step
    I_STATUS,
    I_HAS_LAST,
    I_NEEDS_DISC,
    I_SOLVES,
    I_ITER_COUNT,
    INT_N
};
constexpr int UNUSED_DOUBLES = 8;
constexpr int NMODELS = 3;

__host__ __device__ inline void bind(SCBuffers &b, SCvxBuffers &v, const int *d, const long long *o, int *in, double *arena)
{
    b.B = d[D_B];
    b.K = d[D_K];
    b.x_init_dim = arena + o[O_UNUSED];
    b.X = arena + o[O_X];
    b.U = arena + o[O_U];
    b.sigma = arena + o[O_SIGMA];
    b.ip = arena + o[O_IP];
    b.uhat = b.wtrx = b.sum_delta = b.delta_sigma = arena + o[O_UNUSED];
    b.active = in + I_ACTIVE;
    b.converged = in + I_CONVERGED;
    b.sc_iters = in + I_SC_ITERS;
    b.ipm_iters = in + I_IPM_ITERS;
    b.status = in + I_STATUS;
    b.norm1_nu = arena + o[O_NU1];
    v.Xold = arena + o[O_XOLD];
    v.Uold = arena + o[O_UOLD];
    v.tr = arena + o[O_TR];
    v.last_cost = arena + o[O_LAST];
    v.cost = arena + o[O_COST];
    v.info = arena + o[O_INFO];
    v.has_last = in + I_HAS_LAST;
    v.needs_disc = in + I_NEEDS_DISC;
    v.solves = in + I_SOLVES;
    v.iter_ring = d[D_RING] ? arena + o[O_RING] : nullptr;
    v.iter_count = in + I_ITER_COUNT;
    v.iter_cap = d[D_ITER_CAP];
}

template <class Model, int FORM>
__global__ void __launch_bounds__(WAVE, FORM == 0 ? COST_WAVES_PER_SIMD : IPM_WAVES_PER_SIMD)
    cost_kernel(int count, int model, const int *desc, const long long *offs, int *ints, double *arena, scpp_scvx_opts so)
{
    const int item = blockIdx.x;
    if (item >= count)
        return;
    const int *d = desc + item * DESC_N;
    const long long *o = offs + item * OFF_N;
    if (uniformInt(d[D_MODEL]) != model || uniformInt(d[D_FORM]) != FORM) // another instantiation's job (wave-uniform)
        return;
    SCBuffers b;
    SCvxBuffers v;
    bind(b, v, d, o, ints + item * INT_N, arena);
    if constexpr (FORM == 0)
        scvxCostUpdate<Model>(b, v, so, 0);
    else
    {
        __shared__ double seg_sum[WAVE];
        double *seg = arena + o[O_SEG];
        seg_sum[threadIdx.x] = seg[threadIdx.x];
        WAVE_SYNC();
        scvxCostUpdateSplit<Model>(b, v, so, 0, seg_sum);
        WAVE_SYNC();
        seg[threadIdx.x] = seg_sum[threadIdx.x];
    }
}

// ---- decide kernel: one lane per case.  dbl: tr [n], last_cost [n], norm1_nu [n], the supplied nonlinear cost [n], info [n][4], ip [n][IP_N], cost [n]
//      (not touched by the rule); in: active, converged, sc_iters, status, has_last, needs_disc, solves [n] each, then the returned flags [n]
constexpr int DEC_D = 4 + 4 + IP_N + 1, DEC_I = 8;
__global__ void __launch_bounds__(WAVE) decide_kernel(int n, double *dbl, int *in, scpp_scvx_opts so)
{
    const int c = int(blockIdx.x) * WAVE + int(threadIdx.x);
    if (c >= n)
        return;
    SCBuffers b = {};
    SCvxBuffers v = {};
    b.B = n;
    v.tr = dbl;
    v.last_cost = dbl + n;
    b.norm1_nu = dbl + 2 * n;
    const double *cost_in = dbl + 3 * n;
    v.info = dbl + 4 * n;
    b.ip = dbl + 8 * n;
    v.cost = dbl + (8 + IP_N) * size_t(n);
    b.active = in;
    b.converged = in + n;
    b.sc_iters = in + 2 * n;
    b.status = in + 3 * n;
    v.has_last = in + 4 * n;
    v.needs_disc = in + 5 * n;
    v.solves = in + 6 * n;
    in[7 * n + c] = scvxDecide(b, v, so, c, cost_in[c]);
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

template <class F>
bool withModel(int model, F &&f)
{
    switch (model)
    {
    case SCPP_MODEL_ROCKETQUAT: f(RocketQuatModel{}); return true;
    case SCPP_MODEL_ROCKET2D: f(Rocket2dModel{}); return true;
    case SCPP_MODEL_LANDER3DOF: f(Lander3dofModel{}); return true;
    default: return false;
    }
}

// doubles each block of a job needs; false for a job the step does not admit
bool blockSizes(const int *d, long long *need)
{
    long long nx = 0, nu = 0;
    if (!withModel(d[D_MODEL], [&](auto m) { nx = decltype(m)::NX, nu = decltype(m)::NU; }))
        return false;
    if (d[D_K] < 2 || d[D_K] > WAVE || d[D_FORM] < 0 || d[D_FORM] > 1 || d[D_B] < 0 || d[D_B] > 1 || d[D_ITER_CAP] < 0 || d[D_ITER_CAP] > 64 || d[D_RING] < 0 ||
        d[D_RING] > 1)
        return false;
    const long long K = d[D_K];
    const long long sz[OFF_N] = {K * nx, K * nu, 1, IP_N, 1, K * nx, K * nu, 1, 1, 1, 4, d[D_ITER_CAP] * (long long)scvxIterRecordDoubles(d[D_K], int(nx), int(nu)), WAVE,
                                 UNUSED_DOUBLES};
    for (int f = 0; f < OFF_N; f++)
        need[f] = sz[f];
    return true;
}
bool blocksInside(const int *d, const long long *o, long long arena_doubles)
{
    long long need[OFF_N];
    if (!blockSizes(d, need))
        return false;
    for (int f = 0; f < OFF_N; f++)
        if (o[f] < 0 || o[f] > arena_doubles || need[f] > arena_doubles - o[f])
            return false;
    return true;
}

template <class Model, int FORM>
void launchCost(int count, int model, const int *desc, const long long *offs, int *ints, double *arena, const scpp_scvx_opts &so)
{
    hipLaunchKernelGGL((cost_kernel<Model, FORM>), dim3(count), dim3(WAVE), 0, nullptr, count, model, desc, offs, ints, arena, so);
}

} // namespace

extern "C"
{

int cost_probe_desc_n() { return DESC_N; }
int cost_probe_off_n() { return OFF_N; }
int cost_probe_int_n() { return INT_N; }
const char *cost_probe_off_names() { return "X U sigma ip norm1_nu Xold Uold tr last_cost cost info ring seg unused"; }
const char *cost_probe_int_names() { return "active converged sc_iters ipm_iters status has_last needs_disc solves iter_count"; }
// interface constants a caller must know: IP_N, IP_PAR, IP_TR, SCVX_ITER_SCALARS, SCVX_SOLVE_CAP, SCPP_STATUS_REJECTION_CAP, COST_WAVES_PER_SIMD,
// IPM_WAVES_PER_SIMD, DEC_D, DEC_I
int cost_probe_constants(int *out)
{
    const int c[10] = {IP_N, IP_PAR, IP_TR, SCVX_ITER_SCALARS, SCVX_SOLVE_CAP, SCPP_STATUS_REJECTION_CAP, COST_WAVES_PER_SIMD, IPM_WAVES_PER_SIMD, DEC_D, DEC_I};
    for (int j = 0; j < 10; j++)
        out[j] = c[j];
    return 10;
}
// out = (NX, NU, NP); 0, or 3 for an unknown model
int cost_probe_model_dims(int model, int *out)
{
    return withModel(model, [&](auto m) { out[0] = decltype(m)::NX, out[1] = decltype(m)::NU, out[2] = decltype(m)::NP; }) ? 0 : 3;
}
// need[OFF_N] doubles per block of the job desc[DESC_N]; 0, or 3 for a job the step does not admit
int cost_probe_block_sizes(const int *desc, long long *need) { return blockSizes(desc, need) ? 0 : 3; }

// Runs `count` jobs on the arena and the int fields (copied to the device, copied back whole): one launch per (model, form) that has a job, every launch over
// all blocks.  0; 1: the runtime reported an error; 2: a bad count; 3: a job the step does not admit; 4: a block that does not lie inside the arena
// (nothing is launched then)
int cost_probe_run(int count, const int *desc, const long long *offs, int *ints, double *arena, long long arena_doubles, const scpp_scvx_opts *so)
{
    if (count <= 0 || arena_doubles <= 0 || !so)
        return 2;
    bool has[NMODELS][2] = {};
    for (int q = 0; q < count; q++)
    {
        long long need[OFF_N];
        if (!blockSizes(desc + q * DESC_N, need))
            return 3;
        if (!blocksInside(desc + q * DESC_N, offs + q * OFF_N, arena_doubles))
            return 4;
        has[desc[q * DESC_N + D_MODEL]][desc[q * DESC_N + D_FORM]] = true;
    }
    const size_t bytes = size_t(arena_doubles) * 8, ibytes = size_t(count) * INT_N * sizeof(int);
    Dev ddesc(desc, size_t(count) * DESC_N * sizeof(int)), doffs(offs, size_t(count) * OFF_N * sizeof(long long)), dints(ints, ibytes), darena(arena, bytes);
    if (ddesc.err || doffs.err || dints.err || darena.err)
        return 1;
    const int *dd = static_cast<const int *>(ddesc.p);
    const long long *dofs = static_cast<const long long *>(doffs.p);
    int *di = static_cast<int *>(dints.p);
    double *da = static_cast<double *>(darena.p);
    for (int model = 0; model < NMODELS; model++)
        withModel(model, [&](auto m) {
            using Model = decltype(m);
            if (has[model][0])
                launchCost<Model, 0>(count, model, dd, dofs, di, da, *so);
            if (has[model][1])
                launchCost<Model, 1>(count, model, dd, dofs, di, da, *so);
        });
    const int e1 = hipGetLastError() != hipSuccess, e2 = hipDeviceSynchronize() != hipSuccess;
    if (e1 || e2)
        return 1;
    if (hipMemcpy(ints, dints.p, ibytes, hipMemcpyDeviceToHost) != hipSuccess)
        return 1;
    return hipMemcpy(arena, darena.p, bytes, hipMemcpyDeviceToHost) != hipSuccess ? 1 : 0;
}

// scvx_record_initial_kernel on ONE job (its form is ignored), launched over two blocks: instance 0 and one beyond B.  Return codes as cost_probe_run
int cost_probe_record_initial(const int *desc, const long long *offs, int *ints, double *arena, long long arena_doubles)
{
    if (arena_doubles <= 0)
        return 2;
    long long need[OFF_N];
    if (!blockSizes(desc, need))
        return 3;
    if (!blocksInside(desc, offs, arena_doubles))
        return 4;
    int nx = 0, nu = 0;
    withModel(desc[D_MODEL], [&](auto m) { nx = decltype(m)::NX, nu = decltype(m)::NU; });
    const size_t bytes = size_t(arena_doubles) * 8, ibytes = INT_N * sizeof(int);
    Dev dints(ints, ibytes), darena(arena, bytes);
    if (dints.err || darena.err)
        return 1;
    SCBuffers b;
    SCvxBuffers v;
    bind(b, v, desc, offs, static_cast<int *>(dints.p), static_cast<double *>(darena.p));
    hipLaunchKernelGGL(scvx_record_initial_kernel, dim3(2), dim3(WAVE), 0, nullptr, b, v, nx, nu);
    const int e1 = hipGetLastError() != hipSuccess, e2 = hipDeviceSynchronize() != hipSuccess;
    if (e1 || e2)
        return 1;
    if (hipMemcpy(ints, dints.p, ibytes, hipMemcpyDeviceToHost) != hipSuccess)
        return 1;
    return hipMemcpy(arena, darena.p, bytes, hipMemcpyDeviceToHost) != hipSuccess ? 1 : 0;
}

// scvxDecide on n cases, one lane each: dbl [DEC_D][n] and in [DEC_I][n] as decide_kernel lists them.  0; 1: the runtime reported an error; 2: a bad count
int cost_probe_decide(int n, double *dbl, int *in, const scpp_scvx_opts *so)
{
    if (n <= 0 || !so)
        return 2;
    const size_t bytes = size_t(n) * DEC_D * 8, ibytes = size_t(n) * DEC_I * sizeof(int);
    Dev ddbl(dbl, bytes), din(in, ibytes);
    if (ddbl.err || din.err)
        return 1;
    hipLaunchKernelGGL(decide_kernel, dim3((n + WAVE - 1) / WAVE), dim3(WAVE), 0, nullptr, n, static_cast<double *>(ddbl.p), static_cast<int *>(din.p), *so);
    const int e1 = hipGetLastError() != hipSuccess, e2 = hipDeviceSynchronize() != hipSuccess;
    if (e1 || e2)
        return 1;
    if (hipMemcpy(in, din.p, ibytes, hipMemcpyDeviceToHost) != hipSuccess)
        return 1;
    return hipMemcpy(dbl, ddbl.p, bytes, hipMemcpyDeviceToHost) != hipSuccess ? 1 : 0;
}

} // extern "C"

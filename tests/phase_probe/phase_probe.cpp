// TEST INFRASTRUCTURE ONLY -- never part of the product build.
//
// Probe library for tests/test_phase_residuals.py and tests/test_constraint_rows.py.
//   * phase kernel: the residual pass of scpp_amd/csrc/ipm_solve.h ALONE (phResiduals<P, false>), its fused form (phResiduals<P, true>) and the two
//     phases the fused form claims to equal (phUpdate, then phResiduals<P, false>), each between the two copies of the LDS-resident segment fields
//     (phSegLdsCopy), on record blocks the test has filled;
//   * operator kernel: saff, Lmul and LTmul of scpp_amd/csrc/ipm_kernel.h on one stage per lane;
//   * the constraint table of every model as DATA (cones, rows, terms), and the layout constants a caller of the phases must know.
// No solver code, no copy of a function under test and no arithmetic of its own lives here.
//
// Built by hipcc for gfx950 with the product's flags, a second time with -DRES_PREVLANE_MEMORY=1 (the previous segment's C row by a second load instead
// of the wavefront shift), and by g++ against the wave emulator (__graft_entry__.py).
// Geometry of the phase kernel: the product's (ipm_solve.h: ipmSolveInstance) -- one 64-lane wavefront per block and instance, a __shared__ Ctx, Glob
// and Iter written by lane 0 and handed to the phases by LDS address, dynamic LDS of segLdsBytes<P>(K) for the LDS-resident segment fields; the guard
// item < count and every branch on the job description are wave-uniform.  Instances of different models, policies and horizons share one launch.
// Memory: ONE arena of doubles per launch, copied in, worked on, copied out; a job names its record blocks by offsets into it.  What lies between the
// blocks is the caller's (a sentinel pattern), and the caller sees every byte of it again.  Glob and Iter travel as flat arrays of doubles (the four
// ints of Iter as doubles), in the order of phase_probe_glob_names / phase_probe_iter_names.
#include "../../scpp_amd/csrc/ipm_solve.h"

#include <cstddef>
#include <vector>

namespace
{
using namespace scpp;
using namespace scpp::ipm;

// job description: desc[item][DESC_N] ints, offs[item][OFF_N] offsets (doubles) into the arena
enum Desc
{
    D_MODEL = 0, // 0 RocketQuatSC, 1 Rocket2dSC, 2 Lander3dofSC, 3 ZeroOrderHold<RocketQuatSC>
    D_POLICY,    // 0: nu, nu_b, lam live in LDS ; 1: SegFieldsInWorkspace<...>
    D_K,
    D_OP,        // enum Op
    DESC_N
};
enum Op
{
    OP_RES = 0,   // phSegLdsCopy<P, true> ; phResiduals<P, false> ; phSegLdsCopy<P, false>
    OP_FUSED,     // phSegLdsCopy<P, true> ; phResiduals<P, true> ; phSegLdsCopy<P, false>
    OP_TWO_PHASE, // phSegLdsCopy<P, true> ; phUpdate<P> ; phResiduals<P, false> ; phSegLdsCopy<P, false>
    OP_N
};
enum Offs
{
    O_ST = 0, // [STREC][pitch]
    O_SG,     // [G_NFIELDS * NL][pitch]
    O_DY,     // [DYNREC][pitch]
    O_SX,     // [K][XREC]
    O_IP,     // [IP_N]
    O_GLOB,   // [GLOB_N]
    O_ITER,   // [ITER_N]
    O_UNUSED, // fac, sv, gsave, A .. Z: not used by these phases; they point at a small block of the caller's
    OFF_N
};
constexpr int UNUSED_DOUBLES = 16;
constexpr int NMODELS = 4;

// Glob: doubles only.  Iter: ITER_D doubles, then four ints
constexpr int GLOB_N = int(sizeof(Glob) / sizeof(double));
constexpr int ITER_D = int(offsetof(Iter, D) / sizeof(double));
constexpr int ITER_N = ITER_D + 4;
static_assert(sizeof(Glob) == GLOB_N * sizeof(double) && GLOB_N == 44, "phase_probe_glob_names lists every field of Glob");
static_assert(offsetof(Iter, D) == ITER_D * sizeof(double) && ITER_D == 41, "phase_probe_iter_names lists every field of Iter");

template <class P>
__device__ inline void runPhases(const LDSP Ctx *cs, LDSP Glob *gp, LDSP Iter *itp, int op)
{
    phSegLdsCopy<P, true>(cs);
    if (op == OP_FUSED)
        phResiduals<P, true>(cs, gp, itp);
    else
    {
        if (op == OP_TWO_PHASE)
            phUpdate<P>(cs, gp, itp);
        phResiduals<P, false>(cs, gp, itp);
    }
    phSegLdsCopy<P, false>(cs);
}
template <class P>
__device__ inline void runPolicy(const LDSP Ctx *cs, LDSP Glob *gp, LDSP Iter *itp, int policy, int op)
{
    if (policy == 0)
        runPhases<P>(cs, gp, itp, op);
    else
        runPhases<SegFieldsInWorkspace<P>>(cs, gp, itp, op);
}

// (2: the product's IPM_WAVES_PER_SIMD, ipm_solve.h)
__global__ void __launch_bounds__(WAVE, 2) __attribute__((disable_tail_calls)) phase_kernel(int count, const int *desc, const long long *offs, double *arena)
{
    const int item = blockIdx.x;
    if (item >= count)
        return;
    const int lane = threadIdx.x;
    const int *d = desc + item * DESC_N;
    const long long *o = offs + item * OFF_N;
    const int model = uniformInt(d[D_MODEL]), policy = uniformInt(d[D_POLICY]), op = uniformInt(d[D_OP]);
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
    c.setup_v0 = 0;
    c.st = arena + o[O_ST];
    c.sg = arena + o[O_SG];
    c.dy = arena + o[O_DY];
    c.sx = arena + o[O_SX];
    c.ip = arena + o[O_IP];
    c.fac = c.sv = c.gsave = arena + o[O_UNUSED];
    c.A = c.B = c.C = c.S = c.Z = arena + o[O_UNUSED];
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
    case 0: runPolicy<RocketQuatSC>(cs, gp, itp, policy, op); break;
    case 1: runPolicy<Rocket2dSC>(cs, gp, itp, policy, op); break;
    case 2: runPolicy<Lander3dofSC>(cs, gp, itp, policy, op); break;
    case 3: runPolicy<ZeroOrderHold<RocketQuatSC>>(cs, gp, itp, policy, op); break;
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

// ---- operator kernel: one lane per item; arrays [item][...] doubles, masks[item][2] = (act, fm).  The library pads the device arrays to whole
//      wavefronts with copies of item 0, so the only guard is wave-uniform and no lane is switched off.
//      s_out = saff(ip, act, w, delta, wbar, uhat) ; l_out = Lmul(ip, act, w, delta, uhat) ; (gw, gdl) = LTmul(ip, fm, v, uhat)
constexpr int TPB = 64;
template <class P>
__global__ void __launch_bounds__(TPB) operator_kernel(int n, const double *ip, const unsigned *masks, const double *w, const double *delta, const double *wbar,
                                                       const double *uhat, const double *v, double *s_out, double *l_out, double *gw_out, double *gdl_out)
{
    using L = Lay<P>;
    const int item = int(blockIdx.x) * TPB + int(threadIdx.x);
    if (uniformInt(item & ~63) >= n)
        return;
    const double *ipi = ip + size_t(item) * IP_N;
    const unsigned act = masks[2 * item], fm = masks[2 * item + 1];
    double wk[NV], wb[NV], uh[3], vv[L::NS], so[L::NS], lo[L::NS], gw[NV], gdl;
#pragma unroll
    for (int j = 0; j < NV; j++)
    {
        wk[j] = w[size_t(item) * NV + j];
        wb[j] = wbar[size_t(item) * NV + j];
    }
#pragma unroll
    for (int j = 0; j < 3; j++)
        uh[j] = uhat[size_t(item) * 3 + j];
#pragma unroll
    for (int i = 0; i < L::NS; i++)
        vv[i] = v[size_t(item) * L::NS + i];
    const double dl = delta[item];
    saff<P>(ipi, act, wk, dl, wb, uh, so);
    Lmul<P>(ipi, act, wk, dl, uh, lo);
    LTmul<P>(ipi, fm, vv, uh, gw, &gdl);
#pragma unroll
    for (int i = 0; i < L::NS; i++)
    {
        s_out[size_t(item) * L::NS + i] = so[i];
        l_out[size_t(item) * L::NS + i] = lo[i];
    }
#pragma unroll
    for (int j = 0; j < NV; j++)
        gw_out[size_t(item) * NV + j] = gw[j];
    gdl_out[item] = gdl;
}

// ---- what a caller of the phases must know about a model's records: interface constants, no arithmetic ----
#define LAYOUT_FIELDS(X)                                                                                                                                     \
    X(NX, P::NX) X(NU, P::NU) X(NXV, P::NXV) X(NUV, P::NUV) X(NVU, L::NVU) X(NL, L::NL) X(NS, L::NS) X(LP0, L::LP0) X(NCONES, L::NCONES)                   \
    X(F_W, L::F_W) X(F_DL, L::F_DL) X(F_DW, L::F_DW) X(F_DDL, L::F_DDL) X(F_WBAR, L::F_WBAR) X(F_UHAT, L::F_UHAT) X(F_HDD, L::F_HDD) X(F_HDW, L::F_HDW)   \
    X(F_RXW, L::F_RXW) X(F_RXD, L::F_RXD) X(F_S, L::F_S) X(F_Z, L::F_Z) X(F_DS, L::F_DS) X(F_DZ, L::F_DZ) X(F_RZ, L::F_RZ) X(F_TZ, L::F_TZ)               \
    X(F_LS, L::F_LS) X(F_DSS, L::F_DSS) X(F_ETA, L::F_ETA) X(F_WB, L::F_WB) X(F_BXW, L::F_BXW) X(F_BXD, L::F_BXD) X(F_WBK, L::F_WBK) X(STREC, L::STREC)   \
    X(G_NU, G_NU) X(G_NUB, G_NUB) X(G_S1, G_S1) X(G_Z1, G_Z1) X(G_S2, G_S2) X(G_Z2, G_Z2) X(G_DNU, G_DNU) X(G_DNUB, G_DNUB) X(G_DS1, G_DS1)               \
    X(G_DZ1, G_DZ1) X(G_DS2, G_DS2) X(G_DZ2, G_DZ2) X(G_LAM, G_LAM) X(G_DLAM, G_DLAM) X(G_RY, G_RY) X(G_RXNU, G_RXNU) X(G_RXNUB, G_RXNUB)                 \
    X(G_RZ1, G_RZ1) X(G_RZ2, G_RZ2) X(G_TZ1, G_TZ1) X(G_TZ2, G_TZ2) X(G_QV, G_QV) X(G_BTN, G_BTN) X(G_BNB, G_BNB) X(G_DINV, G_DINV) X(G_CV, G_CV)         \
    X(G_BXNU, G_BXNU) X(G_BXNUB, G_BXNUB) X(G_BY, G_BY) X(G_NFIELDS, G_NFIELDS)                                                                             \
    X(DY_A, L::DY_A) X(DY_B, L::DY_B) X(DY_C, L::DY_C) X(DY_S, L::DY_S) X(DY_Z, L::DY_Z) X(DYNREC, L::DYNREC)                                             \
    X(X_VL, L::X_VL) X(X_BCL, L::X_BCL) X(XREC, L::XREC)                                                                                                     \
    X(IP_GS, IP_GS) X(IP_TILT, IP_TILT) X(IP_WMAX, IP_WMAX) X(IP_TMIN, IP_TMIN) X(IP_TMAX, IP_TMAX) X(IP_GIM, IP_GIM) X(IP_MDRY, IP_MDRY)                 \
    X(IP_WT, IP_WT) X(IP_WTRT, IP_WTRT) X(IP_WTRX, IP_WTRX) X(IP_WVC, IP_WVC) X(IP_SCVX, IP_SCVX) X(IP_TR, IP_TR) X(IP_FIXEDT, IP_FIXEDT) X(IP_N, IP_N)   \
    X(CF_ONE, CF_ONE) X(CF_UHAT0, CF_UHAT0) X(CF_UHAT1, CF_UHAT1) X(CF_UHAT2, CF_UHAT2)                                                                     \
    X(GLOB_N, GLOB_N) X(ITER_N, ITER_N) X(NCONE_APP, P::NCONE) X(NLP, P::NLP)
#define LAYOUT_COUNT_ONE(name, value) +1
#define LAYOUT_NAME_ONE(name, value) #name " "
constexpr int LF_SCALARS = 0 LAYOUT_FIELDS(LAYOUT_COUNT_ONE);
// the scalars, then XMAP [16] and UMAP [16] (-1 beyond NXV / NUV), XINV [16], coneOff [16] and coneDim [16] (cone 0 = the trust-region cone)
constexpr int LF_COUNT = LF_SCALARS + 5 * 16;
// one table row per slack entry of the application cones and the LP rows, in slack order: ints (slot, cone or -1, hpar, var0, coef0, var1, coef1, var2,
// coef2), doubles (hmul, mul0, mul1, mul2)
constexpr int ROW_I = 9, ROW_D = 4, ROWS_MAX = MAXCONES * MAXDIM + MAXLP;

template <class P>
void fillLayout(int *out)
{
    using L = Lay<P>;
    int n = 0;
#define LAYOUT_PUT_ONE(name, value) out[n++] = int(value);
    LAYOUT_FIELDS(LAYOUT_PUT_ONE)
#undef LAYOUT_PUT_ONE
    for (int j = 0; j < 16; j++)
    {
        out[n + j] = j < P::NXV ? P::XMAP[j] : -1;
        out[n + 16 + j] = j < P::NUV ? P::UMAP[j] : -1;
        out[n + 32 + j] = L::XINV.v[j];
        out[n + 48 + j] = L::CONE_OFF.v[j];
        out[n + 64 + j] = L::CONE_DIM.v[j];
    }
}
void putRow(const Row &r, int slot, int cone, int *ri, double *rd)
{
    ri[0] = slot;
    ri[1] = cone;
    ri[2] = r.hpar;
    rd[0] = r.hmul;
    for (int t = 0; t < 3; t++)
    {
        ri[3 + 2 * t] = r.t[t].var;
        ri[4 + 2 * t] = r.t[t].coef;
        rd[1 + t] = r.t[t].mul;
    }
}
template <class P>
int fillTable(int *ri, double *rd)
{
    using D = Derived<P>;
    int n = 0;
    for (int c = 0; c < P::NCONE; c++)
        for (int i = 0; i < P::CONES[c].dim; i++, n++)
            putRow(P::CONES[c].r[i], D::coneOff(c + 1) + i, c + 1, ri + n * ROW_I, rd + n * ROW_D);
    for (int l = 0; l < P::NLP; l++, n++)
        putRow(P::LPS[l], D::LP0 + l, -1, ri + n * ROW_I, rd + n * ROW_D);
    return n;
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
// [count][width] -> [padded][width], the tail filled with copies of item 0
template <class T>
std::vector<T> padded(const T *src, int count, int padded_count, int width)
{
    std::vector<T> v(size_t(padded_count) * width);
    for (int q = 0; q < padded_count; q++)
        for (int i = 0; i < width; i++)
            v[size_t(q) * width + i] = src[size_t(q < count ? q : 0) * width + i];
    return v;
}

template <class P>
int runOperators(int count, const double *ip, const unsigned *masks, const double *w, const double *delta, const double *wbar, const double *uhat, const double *v,
                 double *s_out, double *l_out, double *gw_out, double *gdl_out)
{
    constexpr int NS = Lay<P>::NS;
    const int np = (count + 63) & ~63;
    const auto hip_ = padded(ip, count, np, IP_N);
    const auto hm = padded(masks, count, np, 2);
    const auto hw = padded(w, count, np, NV), hwb = padded(wbar, count, np, NV), hd = padded(delta, count, np, 1), hu = padded(uhat, count, np, 3);
    const auto hv = padded(v, count, np, NS);
    Dev dip(hip_.data(), hip_.size() * 8), dm(hm.data(), hm.size() * 4), dw(hw.data(), hw.size() * 8), dwb(hwb.data(), hwb.size() * 8), dd(hd.data(), hd.size() * 8),
        du(hu.data(), hu.size() * 8), dv(hv.data(), hv.size() * 8);
    Dev ds(nullptr, size_t(np) * NS * 8), dl(nullptr, size_t(np) * NS * 8), dg(nullptr, size_t(np) * NV * 8), dgd(nullptr, size_t(np) * 8);
    if (dip.err || dm.err || dw.err || dwb.err || dd.err || du.err || dv.err || ds.err || dl.err || dg.err || dgd.err)
        return 1;
    hipLaunchKernelGGL(operator_kernel<P>, dim3(np / TPB), dim3(TPB), 0, nullptr, count, static_cast<const double *>(dip.p), static_cast<const unsigned *>(dm.p),
                       static_cast<const double *>(dw.p), static_cast<const double *>(dd.p), static_cast<const double *>(dwb.p), static_cast<const double *>(du.p),
                       static_cast<const double *>(dv.p), static_cast<double *>(ds.p), static_cast<double *>(dl.p), static_cast<double *>(dg.p),
                       static_cast<double *>(dgd.p));
    const int e1 = hipGetLastError() != hipSuccess, e2 = hipDeviceSynchronize() != hipSuccess;
    if (e1 || e2)
        return 1;
    int bad = 0;
    bad |= hipMemcpy(s_out, ds.p, size_t(count) * NS * 8, hipMemcpyDeviceToHost) != hipSuccess;
    bad |= hipMemcpy(l_out, dl.p, size_t(count) * NS * 8, hipMemcpyDeviceToHost) != hipSuccess;
    bad |= hipMemcpy(gw_out, dg.p, size_t(count) * NV * 8, hipMemcpyDeviceToHost) != hipSuccess;
    bad |= hipMemcpy(gdl_out, dgd.p, size_t(count) * 8, hipMemcpyDeviceToHost) != hipSuccess;
    return bad ? 1 : 0;
}

} // namespace

extern "C"
{

// 1: this build takes the previous segment's C row by a second load (RES_PREVLANE_MEMORY, and every emulation build); 0: by the wavefront shift
int phase_probe_prevlane_memory()
{
#if defined(SCPP_HIP_EMU) || RES_PREVLANE_MEMORY
    return 1;
#else
    return 0;
#endif
}

int phase_probe_layout_count() { return LF_COUNT; }
// names of the scalar fields of the layout, in order; XMAP, UMAP, XINV, coneOff and coneDim ([16] each) follow them
const char *phase_probe_layout_names() { return LAYOUT_FIELDS(LAYOUT_NAME_ONE); }
// out[LF_COUNT]; 0, or 3 for an unknown model
int phase_probe_layout(int model, int *out)
{
    return withModel(model, [&](auto p) { fillLayout<decltype(p)>(out); }) ? 0 : 3;
}
// the fields of Glob / Iter in the order of the flat arrays
const char *phase_probe_glob_names()
{
    return "sig dsg n1 sigbar ss zs s3 z3 sc3_0 sc3_1 sc3_2 zc3_0 zc3_1 zc3_2 dsig ddsg dn1 dss dzs ds3 dz3 dsc3_0 dsc3_1 dsc3_2 dzc3_0 dzc3_1 dzc3_2 "
           "seta sw_0 sw_1 sw_2 hsig Hsd Hdd schur lamC_0 lamC_1 lamC_2 dsC_0 dsC_1 dsC_2 dzC_0 dzC_1 dzC_2";
}
const char *phase_probe_iter_names()
{
    return "wtrx w_t w_trt w_vc sigbar gamma resx0 resy0 resz0 mu gap pres dres pcost rzs rz3 rzc_0 rzc_1 rzc_2 rxs rxds rxn1 sigma_c alpha alpha_d tzs "
           "tzc_0 tzc_1 tzc_2 b_s b_ds b_n1 b_rhs3 bts bk_sig bk_dsg bk_n1 pres_prev part_ainv part_ainv_d part_fin D bad bk_valid common_step";
}
double phase_probe_blown() { return IPM_BLOWN; }
int phase_probe_split_steps() { return IPM_SPLIT_STEPS; }

// Lay<P>::fixedMask(k, K) / activeMask(k, K), -1 for an unknown model
int phase_probe_fixed_mask(int model, int k, int K)
{
    int r = -1;
    withModel(model, [&](auto p) { r = int(Lay<decltype(p)>::fixedMask(k, K)); });
    return r;
}
int phase_probe_active_mask(int model, int k, int K)
{
    int r = -1;
    withModel(model, [&](auto p) { r = int(Lay<decltype(p)>::activeMask(k, K)); });
    return r;
}
int phase_probe_rec_pitch(int K) { return recPitch(K); }

// the constraint table as data: ri[ROWS_MAX][9], rd[ROWS_MAX][4] (see ROW_I); returns the number of rows, -1 for an unknown model
int phase_probe_table_rows_max() { return ROWS_MAX; }
int phase_probe_table(int model, int *ri, double *rd)
{
    int n = -1;
    withModel(model, [&](auto p) { n = fillTable<decltype(p)>(ri, rd); });
    return n;
}

// saff, Lmul, LTmul on `count` items of one model (arrays [item][...], see operator_kernel).  0; 1: the runtime reported an error; 2: a bad count;
// 3: an unknown model
int phase_probe_operators(int model, int count, const double *ip, const unsigned *masks, const double *w, const double *delta, const double *wbar,
                          const double *uhat, const double *v, double *s_out, double *l_out, double *gw_out, double *gdl_out)
{
    if (count <= 0)
        return 2;
    int rc = 3;
    withModel(model, [&](auto p) { rc = runOperators<decltype(p)>(count, ip, masks, w, delta, wbar, uhat, v, s_out, l_out, gw_out, gdl_out); });
    return rc;
}

// Runs `count` jobs in ONE launch on the arena (copied to the device, copied back whole).  0; 1: the runtime reported an error; 2: a bad count;
// 3: a job description the phases do not admit; 4: a record block that does not lie inside the arena (nothing is launched then)
int phase_probe_run(int count, const int *desc, const long long *offs, double *arena, long long arena_doubles)
{
    if (count <= 0 || arena_doubles <= 0)
        return 2;
    unsigned lds = 0;
    for (int q = 0; q < count; q++)
    {
        const int *d = desc + q * DESC_N;
        const long long *o = offs + q * OFF_N;
        int lay[LF_COUNT];
        if (phase_probe_layout(d[D_MODEL], lay) != 0 || d[D_K] < 3 || d[D_K] > 64 || d[D_POLICY] < 0 || d[D_POLICY] > 1 || d[D_OP] < 0 || d[D_OP] >= OP_N)
            return 3;
        long long strec = 0, nl = 0, dynrec = 0, xrec = 0;
        withModel(d[D_MODEL], [&](auto p) {
            using L = Lay<decltype(p)>;
            strec = L::STREC, nl = L::NL, dynrec = L::DYNREC, xrec = L::XREC;
            const unsigned b = d[D_POLICY] == 0 ? segLdsBytes<decltype(p)>(d[D_K]) : 0u;
            lds = b > lds ? b : lds;
        });
        const long long K = d[D_K], pitch = recPitch(d[D_K]);
        const long long need[OFF_N] = {strec * pitch, G_NFIELDS * nl * pitch, dynrec * pitch, K * xrec, IP_N, GLOB_N, ITER_N, UNUSED_DOUBLES};
        for (int f = 0; f < OFF_N; f++)
            if (o[f] < 0 || o[f] > arena_doubles || need[f] > arena_doubles - o[f])
                return 4;
    }
    const size_t bytes = size_t(arena_doubles) * 8;
    Dev ddesc(desc, size_t(count) * DESC_N * sizeof(int)), doffs(offs, size_t(count) * OFF_N * sizeof(long long)), darena(arena, bytes);
    if (ddesc.err || doffs.err || darena.err)
        return 1;
    hipLaunchKernelGGL(phase_kernel, dim3(count), dim3(WAVE), lds, nullptr, count, static_cast<const int *>(ddesc.p), static_cast<const long long *>(doffs.p),
                       static_cast<double *>(darena.p));
    const int e1 = hipGetLastError() != hipSuccess, e2 = hipDeviceSynchronize() != hipSuccess;
    if (e1 || e2)
        return 1;
    return hipMemcpy(arena, darena.p, bytes, hipMemcpyDeviceToHost) != hipSuccess ? 1 : 0;
}

} // extern "C"

// TEST INFRASTRUCTURE ONLY -- never part of the product build.
//
// Probe library for tests/test_cone_math.py: thin kernels that call the second-order-cone primitives of scpp_amd/csrc/cone_math.h ONE AT A
// TIME, and the three per-cone stage steps of scpp_amd/csrc/ipm_solve.h (coneScaling, coneT, coneDir) ALONE on stage record blocks the test
// has filled, so that each can be compared with a reference that shares nothing with it (tests/cone_reference.py).  No solver code and no
// copy of a function under test lives here.
//
// Built twice (__graft_entry__.py): by hipcc for gfx950 with the product's flags, and by g++ against the wave emulator.
// Primitive kernels: one lane per item (these are per-lane functions), arrays [item][D] doubles.  The library pads the device arrays to a whole
// number of blocks with copies of item 0, so the only guard is wave-uniform (a wavefront whose first item is past the count returns) and no
// lane is switched off; the caller sees `count` items.
// Stage kernels: one wavefront per instance, lane = stage as in the product, WPB wavefronts per block; the record block of an instance is
// [STREC][recPitch(K)] doubles addressed through makeSV, lanes >= K do nothing.  Every index derives from blockIdx, the wave number and the lane.
#include "../../scpp_amd/csrc/ipm_solve.h"

#include <vector>

namespace
{
using namespace scpp;
using namespace scpp::ipm;

constexpr int TPB = 256; // threads per block of the primitive kernels
constexpr int WPB = 2;   // wavefronts per block of the stage kernels
constexpr int NMODELS = 3;

enum Fn
{
    FN_NT = 0, // a = s, b = z -> out = w, sc = eta, flag = the returned bool (out / sc untouched when it is false)
    FN_W,      // eta, a = w, b = v -> out
    FN_WINV,
    FN_WINV2,
    FN_PROD,   // a = u, b = v -> out
    FN_DIV,    // a = lam, b = dd -> out
    FN_STEP,   // a = lam, b = v -> sc
    FN_N
};

// RT: the runtime-d function (d is a kernel argument), else its compile-time twin
template <int FN, int D, bool RT>
__global__ void __launch_bounds__(TPB) prim_kernel(int n, int d, const double *eta, const double *a, const double *b, double *out, double *sc, int *flag)
{
    const int item = int(blockIdx.x) * TPB + int(threadIdx.x);
    if (uniformInt(item & ~63) >= n)
        return;
    double x[D], y[D], o[D];
#pragma unroll
    for (int i = 0; i < D; i++)
    {
        x[i] = a[size_t(item) * D + i];
        y[i] = b[size_t(item) * D + i];
    }
    if constexpr (FN == FN_NT)
    {
        double e = 0.;
        bool ok;
        if constexpr (RT)
            ok = cone::nt_scaling(x, y, d, e, o);
        else
            ok = cone::nt_scalingS<D>(x, y, e, o);
        flag[item] = ok ? 1 : 0;
        if (ok)
        {
            sc[item] = e;
#pragma unroll
            for (int i = 0; i < D; i++)
                out[size_t(item) * D + i] = o[i];
        }
        return;
    }
    else if constexpr (FN == FN_STEP)
    {
        if constexpr (RT)
            sc[item] = cone::stepInv(d, x, y);
        else
            sc[item] = cone::stepInvS<D>(x, y);
        return;
    }
    else
    {
        const double e = (FN == FN_W || FN == FN_WINV || FN == FN_WINV2) ? eta[item] : 0.;
        if constexpr (FN == FN_W)
        {
            if constexpr (RT)
                cone::applyW(e, x, d, y, o);
            else
                cone::applyWS<D>(e, x, y, o);
        }
        else if constexpr (FN == FN_WINV)
        {
            if constexpr (RT)
                cone::applyWinv(e, x, d, y, o);
            else
                cone::applyWinvS<D>(e, x, y, o);
        }
        else if constexpr (FN == FN_WINV2)
        {
            if constexpr (RT)
                cone::applyWinv2(e, x, d, y, o);
            else
                cone::applyWinv2S<D>(e, x, y, o);
        }
        else if constexpr (FN == FN_PROD)
        {
            if constexpr (RT)
                cone::conicProduct(d, x, y, o);
            else
                cone::conicProductS<D>(x, y, o);
        }
        else
        {
            // in place, as the compile-time function is (the runtime one admits out == dd)
            if constexpr (RT)
                cone::conicDivision(d, x, y, y);
            else
                cone::conicDivisionS<D>(x, y);
#pragma unroll
            for (int i = 0; i < D; i++)
                o[i] = y[i];
        }
#pragma unroll
        for (int i = 0; i < D; i++)
            out[size_t(item) * D + i] = o[i];
    }
}

#define STAGE_ITEM()                                                  \
    const int wave = int(threadIdx.x) >> 6;                           \
    const int lane = int(threadIdx.x) & 63;                           \
    const int item = uniformInt(int(blockIdx.x) * WPB + wave);        \
    if (item >= count)                                                \
        return;                                                       \
    using L = Lay<P>;                                                 \
    const int K = uniformInt(Kin);                                    \
    const int pitch = recPitch(K);                                    \
    const bool on = lane < K;                                         \
    const SV st = makeSV(rec + size_t(item) * L::STREC * pitch, L::STREC, unsigned(on ? lane : 0), pitch); \
    const SV stz = padView(st, uniformInt(scvx) != 0)

// ret[item][lane]: bit C set <=> coneScaling of cone C returned 1
template <class P>
__global__ void __launch_bounds__(64 * WPB) scaling_kernel(int count, int Kin, int scvx, double *rec, int *ret)
{
    STAGE_ITEM();
    if (!on)
        return;
    int bad = 0;
    forEachCone<P>([&](auto ci) {
        constexpr int C = decltype(ci)::value;
        bad |= coneScaling<P, L::coneOff(C), L::coneDim(C)>(st, C, stz) << C;
    });
    ret[item * 64 + lane] = bad;
}

// tout[item][lane < K][LP0]
template <class P>
__global__ void __launch_bounds__(64 * WPB) t_kernel(int count, int Kin, int scvx, int pass_in, const double *om, const double *sigmu, double *rec, double *tout)
{
    STAGE_ITEM();
    if (!on)
        return;
    const int pass = uniformInt(pass_in);
    const double o = om[item], sm = sigmu[item];
    double tzv[L::NS];
    forEachCone<P>([&](auto ci) {
        constexpr int C = decltype(ci)::value;
        coneT<P, L::coneOff(C), L::coneDim(C)>(st, C, pass, o, sm, tzv, stz);
    });
    double *to = tout + (size_t(item) * K + lane) * L::LP0;
#pragma unroll
    for (int i = 0; i < L::LP0; i++)
        to[i] = tzv[i];
}

// Ld[item][lane < K][LP0], ainv0[item][lane < K] (the running maximum each cone starts from), a1 / ainvd[item][lane < K][NCONES]
template <class P>
__global__ void __launch_bounds__(64 * WPB) dir_kernel(int count, int Kin, int scvx, int store_final_in, const double *om, const double *Ld, const double *ainv0,
                                                      double *rec, double *a1, double *ainvd)
{
    STAGE_ITEM();
    if (!on)
        return;
    const bool store_final = uniformInt(store_final_in) != 0;
    const double o = om[item];
    double ld[L::NS];
    const size_t row = size_t(item) * K + lane;
#pragma unroll
    for (int i = 0; i < L::LP0; i++)
        ld[i] = Ld[row * L::LP0 + i];
    const double a0 = ainv0[row];
    forEachCone<P>([&](auto ci) {
        constexpr int C = decltype(ci)::value;
        double ad = a0;
        a1[row * L::NCONES + C] = coneDir<P, L::coneOff(C), L::coneDim(C)>(st, C, o, ld, store_final, stz, ad);
        ainvd[row * L::NCONES + C] = ad;
    });
}

// ---- what a caller of the stage steps must know about a model's stage record: interface constants, no arithmetic ----
enum LayoutField
{
    LF_STREC = 0,
    LF_NS,
    LF_LP0,
    LF_NCONES,
    LF_NXV,
    LF_NVU,
    LF_F_S,
    LF_F_Z,
    LF_F_DS,
    LF_F_DZ,
    LF_F_RZ,
    LF_F_TZ,
    LF_F_LS,
    LF_F_DSS,
    LF_F_ETA,
    LF_F_WB,
    LF_CONE_OFF,                          // [MAXCONES + 1]
    LF_CONE_DIM = LF_CONE_OFF + MAXCONES + 1, // [MAXCONES + 1]
    LF_COUNT = LF_CONE_DIM + MAXCONES + 1
};
template <class P>
void fillLayout(int *out)
{
    using L = Lay<P>;
    out[LF_STREC] = L::STREC;
    out[LF_NS] = L::NS;
    out[LF_LP0] = L::LP0;
    out[LF_NCONES] = L::NCONES;
    out[LF_NXV] = P::NXV;
    out[LF_NVU] = L::NVU;
    out[LF_F_S] = L::F_S;
    out[LF_F_Z] = L::F_Z;
    out[LF_F_DS] = L::F_DS;
    out[LF_F_DZ] = L::F_DZ;
    out[LF_F_RZ] = L::F_RZ;
    out[LF_F_TZ] = L::F_TZ;
    out[LF_F_LS] = L::F_LS;
    out[LF_F_DSS] = L::F_DSS;
    out[LF_F_ETA] = L::F_ETA;
    out[LF_F_WB] = L::F_WB;
    for (int c = 0; c <= MAXCONES; c++)
    {
        out[LF_CONE_OFF + c] = c < L::NCONES ? L::coneOff(c) : -1;
        out[LF_CONE_DIM + c] = c < L::NCONES ? L::coneDim(c) : -1;
    }
}
bool layoutOf(int model, int *out)
{
    switch (model)
    {
    case 0: fillLayout<RocketQuatSC>(out); return true;
    case 1: fillLayout<Rocket2dSC>(out); return true;
    case 2: fillLayout<Lander3dofSC>(out); return true;
    default: return false;
    }
}

struct Dev
{
    void *p = nullptr;
    size_t bytes;
    int err = 0;
    Dev(const void *host, size_t n) : bytes(n)
    {
        if (hipMalloc(&p, bytes ? bytes : 8) != hipSuccess)
            err = 1;
        else if (bytes && host && hipMemcpy(p, host, bytes, hipMemcpyHostToDevice) != hipSuccess)
            err = 1;
    }
    int back(void *host, size_t n) const { return n && hipMemcpy(host, p, n, hipMemcpyDeviceToHost) != hipSuccess; }
    ~Dev()
    {
        if (p)
            (void)hipFree(p);
    }
    template <class T>
    T *as() const
    {
        return static_cast<T *>(p);
    }
};
int finish()
{
    const int e1 = hipGetLastError() != hipSuccess, e2 = hipDeviceSynchronize() != hipSuccess;
    return (e1 || e2) ? 1 : 0;
}

// `count` items of `per` values padded to `padded` items with copies of item 0
template <class T>
std::vector<T> padItems(const T *src, int count, int padded, int per)
{
    std::vector<T> v(size_t(padded) * per);
    for (size_t q = 0; q < v.size(); q++)
        v[q] = q < size_t(count) * per ? src[q] : src[q % size_t(per)];
    return v;
}

template <int FN, int D, bool RT>
int runPrim(int n, const double *eta, const double *a, const double *b, double *out, double *sc, int *flag)
{
    const int padded = (n + TPB - 1) / TPB * TPB;
    const auto he = padItems(eta, n, padded, 1), ha = padItems(a, n, padded, D), hb = padItems(b, n, padded, D);
    const auto ho = padItems(out, n, padded, D), hs = padItems(sc, n, padded, 1);
    const auto hf = padItems(flag, n, padded, 1);
    Dev de(he.data(), he.size() * 8), da(ha.data(), ha.size() * 8), db(hb.data(), hb.size() * 8), dout(ho.data(), ho.size() * 8), dsc(hs.data(), hs.size() * 8),
        df(hf.data(), hf.size() * sizeof(int));
    if (de.err || da.err || db.err || dout.err || dsc.err || df.err)
        return 1;
    auto k = &prim_kernel<FN, D, RT>;
    hipLaunchKernelGGL(k, dim3(padded / TPB), dim3(TPB), 0, nullptr, n, D, de.as<const double>(), da.as<const double>(), db.as<const double>(), dout.as<double>(),
                       dsc.as<double>(), df.as<int>());
    if (finish())
        return 1;
    return (dout.back(out, size_t(n) * D * 8) || dsc.back(sc, size_t(n) * 8) || df.back(flag, size_t(n) * sizeof(int))) ? 1 : 0;
}
template <int FN, bool RT>
int runPrimD(int D, int n, const double *eta, const double *a, const double *b, double *out, double *sc, int *flag)
{
    switch (D)
    {
    case 2: return runPrim<FN, 2, RT>(n, eta, a, b, out, sc, flag);
    case 3: return runPrim<FN, 3, RT>(n, eta, a, b, out, sc, flag);
    case 4: return runPrim<FN, 4, RT>(n, eta, a, b, out, sc, flag);
    case 17: return runPrim<FN, 17, RT>(n, eta, a, b, out, sc, flag);
    default: return 3;
    }
}
template <int FN>
int runPrimFn(int rt, int D, int n, const double *eta, const double *a, const double *b, double *out, double *sc, int *flag)
{
    return rt ? runPrimD<FN, true>(D, n, eta, a, b, out, sc, flag) : runPrimD<FN, false>(D, n, eta, a, b, out, sc, flag);
}

struct StageShape
{
    int lay[LF_COUNT];
    int pitch;
    size_t rec_doubles;
};
// 0, or 2 / 3 for a bad count / model or horizon
int stageShape(int model, int K, int count, StageShape &s)
{
    if (count <= 0)
        return 2;
    if (!layoutOf(model, s.lay) || K < 1 || K > 64)
        return 3;
    s.pitch = recPitch(K);
    s.rec_doubles = size_t(count) * s.lay[LF_STREC] * s.pitch;
    return 0;
}
dim3 stageGrid(int count) { return dim3((count + WPB - 1) / WPB); }

template <class P>
void launchScaling(int count, int K, int scvx, double *rec, int *ret)
{
    auto k = &scaling_kernel<P>;
    hipLaunchKernelGGL(k, stageGrid(count), dim3(64 * WPB), 0, nullptr, count, K, scvx, rec, ret);
}
template <class P>
void launchT(int count, int K, int scvx, int pass, const double *om, const double *sigmu, double *rec, double *tout)
{
    auto k = &t_kernel<P>;
    hipLaunchKernelGGL(k, stageGrid(count), dim3(64 * WPB), 0, nullptr, count, K, scvx, pass, om, sigmu, rec, tout);
}
template <class P>
void launchDir(int count, int K, int scvx, int store_final, const double *om, const double *Ld, const double *ainv0, double *rec, double *a1, double *ainvd)
{
    auto k = &dir_kernel<P>;
    hipLaunchKernelGGL(k, stageGrid(count), dim3(64 * WPB), 0, nullptr, count, K, scvx, store_final, om, Ld, ainv0, rec, a1, ainvd);
}

} // namespace

extern "C"
{

int cone_probe_layout_count() { return LF_COUNT; }

// names of the scalar fields of the layout, in the order of enum LayoutField; CONE_OFF [7] and CONE_DIM [7] (-1 beyond NCONES) follow them
const char *cone_probe_layout_names() { return "STREC NS LP0 NCONES NXV NVU F_S F_Z F_DS F_DZ F_RZ F_TZ F_LS F_DSS F_ETA F_WB"; }

// out[LF_COUNT]; 0, or 3 for an unknown model
int cone_probe_layout(int model, int *out) { return layoutOf(model, out) ? 0 : 3; }

int cone_probe_rec_pitch(int K) { return recPitch(K); }

// One primitive (enum Fn) on n items of dimension D in {2, 3, 4, 17}; rt != 0: the runtime-d function.  eta[n], a / b / out[n][D], sc[n], flag[n];
// what a function does not write keeps the caller's contents.  0; 1: the runtime reported an error; 2: a bad count; 3: an unknown function or dimension
int cone_probe_prim(int fn, int rt, int D, int n, const double *eta, const double *a, const double *b, double *out, double *sc, int *flag)
{
    if (n <= 0)
        return 2;
    switch (fn)
    {
    case FN_NT: return runPrimFn<FN_NT>(rt, D, n, eta, a, b, out, sc, flag);
    case FN_W: return runPrimFn<FN_W>(rt, D, n, eta, a, b, out, sc, flag);
    case FN_WINV: return runPrimFn<FN_WINV>(rt, D, n, eta, a, b, out, sc, flag);
    case FN_WINV2: return runPrimFn<FN_WINV2>(rt, D, n, eta, a, b, out, sc, flag);
    case FN_PROD: return runPrimFn<FN_PROD>(rt, D, n, eta, a, b, out, sc, flag);
    case FN_DIV: return runPrimFn<FN_DIV>(rt, D, n, eta, a, b, out, sc, flag);
    case FN_STEP: return runPrimFn<FN_STEP>(rt, D, n, eta, a, b, out, sc, flag);
    default: return 3;
    }
}

// coneScaling of every cone of the model on rec[count][STREC][recPitch(K)] (copied in, worked on, copied back whole); ret[count][64], lanes >= K untouched
int cone_probe_scaling(int model, int K, int scvx, int count, double *rec, int *ret)
{
    StageShape s;
    if (const int e = stageShape(model, K, count, s))
        return e;
    Dev drec(rec, s.rec_doubles * 8), dret(ret, size_t(count) * 64 * sizeof(int));
    if (drec.err || dret.err)
        return 1;
    switch (model)
    {
    case 0: launchScaling<RocketQuatSC>(count, K, scvx, drec.as<double>(), dret.as<int>()); break;
    case 1: launchScaling<Rocket2dSC>(count, K, scvx, drec.as<double>(), dret.as<int>()); break;
    default: launchScaling<Lander3dofSC>(count, K, scvx, drec.as<double>(), dret.as<int>()); break;
    }
    if (finish())
        return 1;
    return (drec.back(rec, drec.bytes) || dret.back(ret, dret.bytes)) ? 1 : 0;
}

// coneT of every cone; om[count], sigmu[count], tout[count][K][LP0]
int cone_probe_t(int model, int K, int scvx, int count, int pass, const double *om, const double *sigmu, double *rec, double *tout)
{
    StageShape s;
    if (const int e = stageShape(model, K, count, s))
        return e;
    if (pass < 0 || pass > 1)
        return 3;
    Dev drec(rec, s.rec_doubles * 8), dom(om, size_t(count) * 8), dsm(sigmu, size_t(count) * 8), dt(tout, size_t(count) * K * s.lay[LF_LP0] * 8);
    if (drec.err || dom.err || dsm.err || dt.err)
        return 1;
    switch (model)
    {
    case 0: launchT<RocketQuatSC>(count, K, scvx, pass, dom.as<const double>(), dsm.as<const double>(), drec.as<double>(), dt.as<double>()); break;
    case 1: launchT<Rocket2dSC>(count, K, scvx, pass, dom.as<const double>(), dsm.as<const double>(), drec.as<double>(), dt.as<double>()); break;
    default: launchT<Lander3dofSC>(count, K, scvx, pass, dom.as<const double>(), dsm.as<const double>(), drec.as<double>(), dt.as<double>()); break;
    }
    if (finish())
        return 1;
    return (drec.back(rec, drec.bytes) || dt.back(tout, dt.bytes)) ? 1 : 0;
}

// coneDir of every cone; om[count], Ld[count][K][LP0], ainv0[count][K], a1 / ainvd[count][K][NCONES]
int cone_probe_dir(int model, int K, int scvx, int count, int store_final, const double *om, const double *Ld, const double *ainv0, double *rec, double *a1,
                   double *ainvd)
{
    StageShape s;
    if (const int e = stageShape(model, K, count, s))
        return e;
    const size_t rows = size_t(count) * K;
    Dev drec(rec, s.rec_doubles * 8), dom(om, size_t(count) * 8), dld(Ld, rows * s.lay[LF_LP0] * 8), da0(ainv0, rows * 8), da1(a1, rows * s.lay[LF_NCONES] * 8),
        dad(ainvd, rows * s.lay[LF_NCONES] * 8);
    if (drec.err || dom.err || dld.err || da0.err || da1.err || dad.err)
        return 1;
    switch (model)
    {
    case 0:
        launchDir<RocketQuatSC>(count, K, scvx, store_final, dom.as<const double>(), dld.as<const double>(), da0.as<const double>(), drec.as<double>(), da1.as<double>(),
                                dad.as<double>());
        break;
    case 1:
        launchDir<Rocket2dSC>(count, K, scvx, store_final, dom.as<const double>(), dld.as<const double>(), da0.as<const double>(), drec.as<double>(), da1.as<double>(),
                              dad.as<double>());
        break;
    default:
        launchDir<Lander3dofSC>(count, K, scvx, store_final, dom.as<const double>(), dld.as<const double>(), da0.as<const double>(), drec.as<double>(), da1.as<double>(),
                                dad.as<double>());
        break;
    }
    if (finish())
        return 1;
    return (drec.back(rec, drec.bytes) || da1.back(a1, da1.bytes) || dad.back(ainvd, dad.bytes)) ? 1 : 0;
}

} // extern "C"

// TEST INFRASTRUCTURE ONLY -- never part of the product build.
//
// Probe library for tests/test_tile_engine.py: thin kernels that call the functions of scpp_amd/csrc/tile_engine.h and the lane
// primitives of scpp_amd/csrc/common.h ONE AT A TIME, on dense arrays, so that each can be compared with a reference that shares
// nothing with it (tests/tile_reference.py).  No solver code and no copy of a function under test lives here.
//
// Built twice (__graft_entry__.py): by hipcc for gfx950 with the product's flags, and by g++ against the wave emulator.
// Geometry of every kernel: one wavefront per item, WPB wavefronts per block, each with its own TileShared (as the product has
// several wavefronts sharing one LDS); a wave-uniform guard item < count; every index derived from blockIdx, the wave number and
// the lane only; inputs and outputs are dense arrays sized by count.
#include "../../scpp_amd/csrc/tile_engine.h"

#include <cstring>

namespace
{
using namespace scpp;
using namespace scpp::ipm;

constexpr int WPB = 4; // wavefronts per block

#define PROBE_ITEM()                                            \
    const int wave = int(threadIdx.x) >> 6;                     \
    const int lane = int(threadIdx.x) & 63;                     \
    const int item = int(blockIdx.x) * WPB + wave;              \
    if (item >= count)                                          \
        return;

__device__ inline double bitsToDouble(unsigned long long b)
{
    double d;
    __builtin_memcpy(&d, &b, 8);
    return d;
}
__device__ inline unsigned long long doubleToBits(double d)
{
    unsigned long long b;
    __builtin_memcpy(&b, &d, 8);
    return b;
}

// ---- lane moves: 64 bit patterns in, 64 out, through the move `ops[item]` ----
// 0 rowXor1, 1 rowXor2, 2 rowHalfMirror, 3 rowMirror, 4 rowRor8, 5 pairHead, 6 prevLane, 7 rowGroupDiag, 8 + GS rowGroupBcast<GS>,
// 16 + J rowBcast<J>, 64 + s readLane(., s)
__global__ void __launch_bounds__(64 * WPB) lane_move_kernel(int count, const int *ops, const unsigned long long *in, unsigned long long *out)
{
    PROBE_ITEM();
    const int op = uniformInt(ops[item]);
    const double v = bitsToDouble(in[item * 64 + lane]);
    double o = 0.;
    switch (op)
    {
    case 0: o = rowXor1(v); break;
    case 1: o = rowXor2(v); break;
    case 2: o = rowHalfMirror(v); break;
    case 3: o = rowMirror(v); break;
    case 4: o = rowRor8(v); break;
    case 5: o = pairHead(v); break;
    case 6: o = prevLane(v); break;
    case 7: o = rowGroupDiag(v); break;
    case 8: o = rowGroupBcast<0>(v); break;
    case 9: o = rowGroupBcast<1>(v); break;
    case 10: o = rowGroupBcast<2>(v); break;
    case 11: o = rowGroupBcast<3>(v); break;
    case 16: o = rowBcast<0>(v); break;
    case 17: o = rowBcast<1>(v); break;
    case 18: o = rowBcast<2>(v); break;
    case 19: o = rowBcast<3>(v); break;
    case 20: o = rowBcast<4>(v); break;
    case 21: o = rowBcast<5>(v); break;
    case 22: o = rowBcast<6>(v); break;
    case 23: o = rowBcast<7>(v); break;
    case 24: o = rowBcast<8>(v); break;
    case 25: o = rowBcast<9>(v); break;
    case 26: o = rowBcast<10>(v); break;
    case 27: o = rowBcast<11>(v); break;
    case 28: o = rowBcast<12>(v); break;
    case 29: o = rowBcast<13>(v); break;
    case 30: o = rowBcast<14>(v); break;
    case 31: o = rowBcast<15>(v); break;
    default:
        if (op >= 64 && op < 128)
            o = readLane(v, op - 64);
        break;
    }
    out[item * 64 + lane] = doubleToBits(o);
}

__global__ void __launch_bounds__(64 * WPB) any_lane_kernel(int count, const int *pred, int *out)
{
    PROBE_ITEM();
    out[item * 64 + lane] = anyLane(pred[item * 64 + lane] != 0) ? 1 : 0;
}

// ---- reductions: out[item][q][lane], q = rowSum16, rowMax16, waveSumDpp, wave_sum, waveMaxDpp, wave_max ----
__global__ void __launch_bounds__(64 * WPB) reduce_kernel(int count, const double *in, double *out)
{
    PROBE_ITEM();
    const double v = in[item * 64 + lane];
    double *o = out + size_t(item) * 6 * 64 + lane;
    o[0 * 64] = rowSum16(v);
    o[1 * 64] = rowMax16(v);
    o[2 * 64] = waveSumDpp(v);
    o[3 * 64] = wave_sum(v);
    o[4 * 64] = waveMaxDpp(v);
    o[5 * 64] = wave_max(v);
}

// ---- fastRcp / fastRsqrt, elementwise: item = 64 consecutive arguments ----
__global__ void __launch_bounds__(64 * WPB) rcp_kernel(int count, const double *in, double *rcp, double *rsq)
{
    PROBE_ITEM();
    const double d = in[item * 64 + lane];
    rcp[item * 64 + lane] = fastRcp(d);
    rsq[item * 64 + lane] = fastRsqrt(d);
}

// ---- mm: C0 = mm(loadTile X, loadTile Y), C1 = mm(loadTileT X, loadTileT Y) ----
__global__ void __launch_bounds__(64 * WPB) mm_kernel(int count, const double *X, const double *Y, double *C0, double *C1)
{
    PROBE_ITEM();
    const double *x = X + size_t(item) * 256, *y = Y + size_t(item) * 256;
    storeTile(C0 + size_t(item) * 256, lane, mm(loadTile(x, lane), loadTile(y, lane)));
    storeTile(C1 + size_t(item) * 256, lane, mm(loadTileT(x, lane), loadTileT(y, lane)));
}

// ---- loads and transposes: out[item][q], q = storeTile(loadTile), storeTile(loadTileT), transposeTile, transposeTileMfma ----
__global__ void __launch_bounds__(64 * WPB) transpose_kernel(int count, const double *X, double *out)
{
    PROBE_ITEM();
    __shared__ TileShared shAll[WPB];
    TileShared &sh = shAll[wave];
    const double *x = X + size_t(item) * 256;
    double *o = out + size_t(item) * 4 * 256;
    const Tile t = loadTile(x, lane);
    storeTile(o, lane, t);
    storeTile(o + 256, lane, loadTileT(x, lane));
    storeTile(o + 512, lane, transposeTile(t, sh, lane));
    storeTile(o + 768, lane, transposeTileMfma(t, lane));
}

// ---- mv: y1 = mv(T, x), y2 = mv(T2, mv(T, x)); all 64 lane values of both ----
__global__ void __launch_bounds__(64 * WPB) mv_kernel(int count, const double *T, const double *T2, const double *x, double *y1, double *y2)
{
    PROBE_ITEM();
    const Tile t = loadTile(T + size_t(item) * 256, lane), t2 = loadTile(T2 + size_t(item) * 256, lane);
    const double xv = x[item * 16 + vElem(lane)];
    const double a = mv(t, xv);
    y1[item * 64 + lane] = a;
    y2[item * 64 + lane] = mv(t2, a);
}

// ---- eliminations: out[item][q], q = invCholImpl<n, false>, invCholImpl<n, true>, invCholFactor<n>, invCholFactorT<n>; ok[item] ----
template <int n>
__global__ void __launch_bounds__(64 * WPB) invchol_kernel(int count, const double *A, double *out, int *okOut)
{
    PROBE_ITEM();
    __shared__ TileShared shAll[WPB];
    TileShared &sh = shAll[wave];
    const Tile a = loadTile(A + size_t(item) * 256, lane);
    double *o = out + size_t(item) * 4 * 256;
    bool ok = true, unused = true;
    storeTile(o, lane, invCholImpl<n, false>(a, sh, lane, &ok));
    storeTile(o + 256, lane, invCholImpl<n, true>(a, sh, lane, &unused));
    storeTile(o + 512, lane, invCholFactor<n>(a, sh, lane));
    storeTile(o + 768, lane, invCholFactorT<n>(a, lane));
    if (lane == 0)
        okOut[item] = ok ? 1 : 0;
}

// ---- host side: copy in, launch, copy out ----
struct Dev
{
    void *p = nullptr;
    void *host;
    size_t bytes;
    bool out;
    int err = 0;
    Dev(void *h, size_t b, bool o) : host(h), bytes(b), out(o)
    {
        if (hipMalloc(&p, b ? b : 8) != hipSuccess)
            err = 1;
        else if (!out && b && hipMemcpy(p, host, b, hipMemcpyHostToDevice) != hipSuccess)
            err = 1;
    }
    int finish()
    {
        if (!err && out && bytes && hipMemcpy(host, p, bytes, hipMemcpyDeviceToHost) != hipSuccess)
            err = 1;
        return err;
    }
    ~Dev()
    {
        if (p)
            (void)hipFree(p);
    }
    template <class T>
    T *as() { return static_cast<T *>(p); }
};
inline int blocks(int count) { return (count + WPB - 1) / WPB; }
inline int synced()
{
    const int e1 = hipGetLastError() != hipSuccess, e2 = hipDeviceSynchronize() != hipSuccess;
    return e1 || e2;
}
#define PROBE_LAUNCH(kernel, count, ...) hipLaunchKernelGGL(kernel, dim3(blocks(count)), dim3(64 * WPB), 0, nullptr, count, __VA_ARGS__)

} // namespace

// every launcher returns 0, or nonzero when the runtime reported an error; count <= 0 is an error
extern "C"
{

int tile_probe_lane_move(int count, const int *ops, const unsigned long long *in, unsigned long long *out)
{
    if (count <= 0)
        return 2;
    Dev dops(const_cast<int *>(ops), size_t(count) * sizeof(int), false), din(const_cast<unsigned long long *>(in), size_t(count) * 64 * 8, false),
        dout(out, size_t(count) * 64 * 8, true);
    if (dops.err || din.err || dout.err)
        return 1;
    PROBE_LAUNCH(lane_move_kernel, count, dops.as<const int>(), din.as<const unsigned long long>(), dout.as<unsigned long long>());
    return synced() || dout.finish();
}

int tile_probe_any_lane(int count, const int *pred, int *out)
{
    if (count <= 0)
        return 2;
    Dev din(const_cast<int *>(pred), size_t(count) * 64 * sizeof(int), false), dout(out, size_t(count) * 64 * sizeof(int), true);
    if (din.err || dout.err)
        return 1;
    PROBE_LAUNCH(any_lane_kernel, count, din.as<const int>(), dout.as<int>());
    return synced() || dout.finish();
}

int tile_probe_reduce(int count, const double *in, double *out)
{
    if (count <= 0)
        return 2;
    Dev din(const_cast<double *>(in), size_t(count) * 64 * 8, false), dout(out, size_t(count) * 6 * 64 * 8, true);
    if (din.err || dout.err)
        return 1;
    PROBE_LAUNCH(reduce_kernel, count, din.as<const double>(), dout.as<double>());
    return synced() || dout.finish();
}

int tile_probe_rcp(int count, const double *in, double *rcp, double *rsq)
{
    if (count <= 0)
        return 2;
    const size_t b = size_t(count) * 64 * 8;
    Dev din(const_cast<double *>(in), b, false), d1(rcp, b, true), d2(rsq, b, true);
    if (din.err || d1.err || d2.err)
        return 1;
    PROBE_LAUNCH(rcp_kernel, count, din.as<const double>(), d1.as<double>(), d2.as<double>());
    return synced() || d1.finish() || d2.finish();
}

int tile_probe_mm(int count, const double *X, const double *Y, double *C0, double *C1)
{
    if (count <= 0)
        return 2;
    const size_t b = size_t(count) * 256 * 8;
    Dev dx(const_cast<double *>(X), b, false), dy(const_cast<double *>(Y), b, false), d0(C0, b, true), d1(C1, b, true);
    if (dx.err || dy.err || d0.err || d1.err)
        return 1;
    PROBE_LAUNCH(mm_kernel, count, dx.as<const double>(), dy.as<const double>(), d0.as<double>(), d1.as<double>());
    return synced() || d0.finish() || d1.finish();
}

int tile_probe_transpose(int count, const double *X, double *out)
{
    if (count <= 0)
        return 2;
    const size_t b = size_t(count) * 256 * 8;
    Dev dx(const_cast<double *>(X), b, false), dout(out, 4 * b, true);
    if (dx.err || dout.err)
        return 1;
    PROBE_LAUNCH(transpose_kernel, count, dx.as<const double>(), dout.as<double>());
    return synced() || dout.finish();
}

int tile_probe_mv(int count, const double *T, const double *T2, const double *x, double *y1, double *y2)
{
    if (count <= 0)
        return 2;
    const size_t b = size_t(count) * 256 * 8, bv = size_t(count) * 64 * 8;
    Dev dt(const_cast<double *>(T), b, false), dt2(const_cast<double *>(T2), b, false), dx(const_cast<double *>(x), size_t(count) * 16 * 8, false),
        d1(y1, bv, true), d2(y2, bv, true);
    if (dt.err || dt2.err || dx.err || d1.err || d2.err)
        return 1;
    PROBE_LAUNCH(mv_kernel, count, dt.as<const double>(), dt2.as<const double>(), dx.as<const double>(), d1.as<double>(), d2.as<double>());
    return synced() || d1.finish() || d2.finish();
}

// n in {1, 4, 5, 6, 7, 13, 14, 16}: the product's sizes (6, 7, 14, 16) and the sizes next to a register-row boundary; another n: 3
int tile_probe_invchol(int n, int count, const double *A, double *out, int *ok)
{
    if (count <= 0)
        return 2;
    const size_t b = size_t(count) * 256 * 8;
    Dev da(const_cast<double *>(A), b, false), dout(out, 4 * b, true), dok(ok, size_t(count) * sizeof(int), true);
    if (da.err || dout.err || dok.err)
        return 1;
#define PROBE_INVCHOL(N)                                                                                       \
    case N:                                                                                                    \
        PROBE_LAUNCH(invchol_kernel<N>, count, da.as<const double>(), dout.as<double>(), dok.as<int>());       \
        break;
    switch (n)
    {
        PROBE_INVCHOL(1)
        PROBE_INVCHOL(4)
        PROBE_INVCHOL(5)
        PROBE_INVCHOL(6)
        PROBE_INVCHOL(7)
        PROBE_INVCHOL(13)
        PROBE_INVCHOL(14)
        PROBE_INVCHOL(16)
    default:
        return 3;
    }
#undef PROBE_INVCHOL
    return synced() || dout.finish() || dok.finish();
}

} // extern "C"

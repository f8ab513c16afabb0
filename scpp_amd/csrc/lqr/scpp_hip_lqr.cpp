// C ABI of the batched LQR tracker (include/scpp_hip_lqr.h): context, buffers and launches for the kernels of csrc/lqr/.
// Built as a library of its own (libscpp_lqr.so; with -DSCPP_HIP_EMU: the CPU emulation of the same source), see DESIGN.md 4.8.
#include "../../../include/scpp_hip_lqr.h"
#include "lqr_kernels.h"
#include "lqr_riccati_kernel.h"
#include "lqr_covariance_kernel.h"
#include "lqr_discrete_kernel.h"
#include "lqr_covariance_discrete_kernel.h"
#include "lqr_sweep_launch.h"

#ifdef SCPP_HIP_EMU
#include "scpp_hip_lqr_affine.cpp" // the emulation is one translation unit (its fiber switch is a global symbol of the emulation header)
#include "scpp_hip_lqr_moments.cpp"
#include "scpp_hip_lqr_filter.cpp"
#endif

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>

using namespace scpp;
using namespace scpp::lqr;

#define CHECK_HIP(expr)        \
    do                         \
    {                          \
        if ((expr) != hipSuccess) \
            return SCPP_E_HIP; \
    } while (0)

// THE VALIDITY FLAGS: which entry point clears and sets which (everything else leaves them alone).  "products" = have_p, have_disc and the
// trio have_ff / have_affine / affine_kept (clearGainProducts); "trio" = the three alone (clearAffineProducts).
//
//   entry point                                   clears                                              sets
//   set_trajectories, set_trajectories_device     have_gains, gains_computed, products, have_cov      have_traj                    (invalidateGains)
//   set_gains                                     have_gains, gains_computed, products, have_cov      then have_gains              (invalidateGains)
//   set_weights, set_terminal_weights             if gains_computed: as set_trajectories              (have_qf)                    (invalidateComputedGains)
//   set_flow_params                               have_cov, trio; if gains_computed: as above         have_par
//   compute_gains                  after launch:  products, have_cov                                  have_gains, gains_computed
//   compute_gains_riccati          before growTo: products;  after launch: have_cov                   have_gains, gains_computed, have_p = keep
//   compute_gains_affine           before growTo: products;  after launch: have_cov                   have_gains, gains_computed, have_ff, have_affine,
//                                                                                                     affine_kept = keep
//   compute_gains_discrete         before growTo: products;  after launch: have_cov                   have_gains, gains_computed, have_disc = keep
//   set_feedforward_terms                         have_affine, affine_kept                            have_ff
//   set_covariance_inputs                         have_cov                                            have_cov_in
//   propagate_covariance(_discrete) before growTo: have_cov, have_mom                                 after launch: have_cov, cov_kept = keep
//   propagate_moments              before growTo: have_cov, have_mom                                  after launch: have_cov, have_mom, cov_kept = keep
//   set_measurement                               have_filt                                           have_meas (H == NULL: cleared)
//   filter                         before growTo: have_filt                                           after launch: have_filt, filt_loop = closed_loop,
//                                                                                                     filt_kept = keep
//   have_filt is also cleared by whatever changes the trajectories, the parameters or the covariance inputs and, when filt_loop, by whatever
//   changes the gains (clearFilterResult, clearLoopFilterResult); the covariance and moments sweeps leave it alone, and the filter sweep them.
//   track, track_samples                          have_track, if the flight buffers had to grow       after the flights: have_track
//   set_disturbance, disturbance_normals          nothing                                             nothing (have_noise is a setting, not a result)
//
// A call that fails before the point named leaves the flags as they were; one that fails after it (a failed growTo, a failed launch) leaves
// them cleared and sets nothing.
struct scpp_hip_lqr_ctx
{
    int device = 0, model = 0, K = 0, nU = 0, uRows = 0, Bmax = 0, B = 0;
    int par_rows = 0; // rows given to scpp_hip_lqr_set_flow_params: 1 (shared) or the number of trajectories
    int nx = 0, nu = 0, np = 0, nr = 0;
    hipStream_t stream = nullptr;
    double *X = nullptr, *U = nullptr, *T = nullptr;          // owned copies (scpp_hip_lqr_set_trajectories)
    const double *tX = nullptr, *tU = nullptr, *tT = nullptr; // the trajectories in use: the owned copies or the caller's device memory
    double *par = nullptr, *q = nullptr, *r = nullptr, *G = nullptr;
    double *qf = nullptr, *P = nullptr; // terminal weights (used when have_qf) and P(t_k) of the last Riccati sweep, allocated on request only
    size_t P_cap = 0;                   // doubles allocated behind P
    bool have_qf = false, have_p = false;
    // discrete sweep (scpp_hip_lqr_compute_gains_discrete): P lands in the buffer above, Phi and Gamma of every segment in two of their own,
    // allocated by the first keep request
    double *phi = nullptr, *gam = nullptr;
    size_t phi_cap = 0, gam_cap = 0;
    bool have_disc = false;
    int hold = 0; // scpp_hip_lqr_set_feedback_hold
    // affine sweep (scpp_hip_lqr_compute_gains_affine): the feedforward terms k_k, allocated by the first sweep or the first
    // scpp_hip_lqr_set_feedforward_terms; P lands in the buffer above, p and s in two of their own, allocated by the first keep request
    double *ff = nullptr, *ap = nullptr, *as = nullptr;
    size_t ff_cap = 0, ap_cap = 0, as_cap = 0;
    bool have_ff = false, have_affine = false, affine_kept = false; // terms held; the last gain computation was the affine sweep; with keep
    int ffmode = 0;                                                  // scpp_hip_lqr_set_feedforward
    int *gstatus = nullptr, *giters = nullptr;
    // covariance sweep (scpp_hip_lqr_propagate_covariance): inputs and outputs are allocated by the first scpp_hip_lqr_set_covariance_inputs,
    // the full S(t_k) by the first keep_cov request
    double *s0 = nullptr, *cw = nullptr, *cstd = nullptr, *cin = nullptr, *cfin = nullptr, *cov = nullptr;
    int *cstatus = nullptr;
    size_t cov_cap = 0;
    int s0_rows = 0; // rows given to scpp_hip_lqr_set_covariance_inputs: 1 (shared) or the number of trajectories
    bool have_cov_in = false, have_cov = false, cov_kept = false;
    // moments sweep (scpp_hip_lqr_propagate_moments): the covariance part lands in the buffers above; mean0, m(t_k) and du_mean[k] in three of
    // their own, allocated by the first sweep
    double *m0 = nullptr, *cmean = nullptr, *cdu = nullptr;
    bool have_mom = false; // the last sweep was the moments sweep (read together with have_cov, which everything that invalidates a sweep clears)
    // filter sweep (scpp_hip_lqr_filter): the measurement (H [ny][nx], v [ny]; room for 16 rows) is allocated by the first
    // scpp_hip_lqr_set_measurement, the outputs by the first sweep, the loop's by the first sweep with closed_loop, the kept tiles on request
    double *mH = nullptr, *mv = nullptr;
    int ny = 0;
    double *fL = nullptr, *fes = nullptr, *ffe = nullptr, *fec = nullptr, *fss = nullptr, *fic = nullptr, *ffs = nullptr, *fxc = nullptr;
    int *fstatus = nullptr;
    size_t fec_cap = 0, fxc_cap = 0;
    bool have_meas = false, have_filt = false, filt_loop = false, filt_kept = false;
    double *xs = nullptr, *xf = nullptr, *ox = nullptr, *ou = nullptr, *os = nullptr;
    int *oi = nullptr;
    double *rx = nullptr, *ru = nullptr, *rt = nullptr;
    int *rn = nullptr;
    int n_record = 0, rec_cap = 0, rec_alloc_rows = 0, rec_alloc_inst = 0;
    int par_stride = 0;
    bool have_par = false, have_traj = false, have_gains = false, gains_computed = false, have_track = false;
    int track_B = 0;
    double stop_tol = 0.;
    // flights: xs, ox, ou, os, oi and the two saturation outputs hold fl_cap flights (batch_max at first, grown on demand by a sample fan)
    size_t fl_cap = 0;
    int *onsat = nullptr;
    double *oclip = nullptr;
    // input limits (scpp_hip_lqr_set_input_limits): rows of LIM_ROW doubles, allocated by the first call that sets some
    double *lim = nullptr;
    int lim_rows = 0; // 1 (shared) or the number of trajectories
    bool have_lim = false;
    // process noise (scpp_hip_lqr_set_disturbance): the intensities stay on the host; every flight call turns them into sqrt(w / time_step)
    // with its own time step (noise_sd, which lives as long as the context because it is copied asynchronously) and uploads that row to nsd,
    // allocated by the first call that sets some
    static constexpr int NOISE_MAX_NX = 32;
    double noise_w[NOISE_MAX_NX] = {}, noise_sd[NOISE_MAX_NX] = {};
    double *nsd = nullptr;
    unsigned long long noise_seed = 0, noise_offset = 0;
    bool have_noise = false;
};

template <class T>
static int devAlloc(T **p, size_t n)
{
    return hipMalloc(reinterpret_cast<void **>(p), (n ? n : 1) * sizeof(T)) == hipSuccess ? 0 : 1;
}

struct DeviceGuard
{
    int prev = -1;
    explicit DeviceGuard(int want)
    {
        (void)hipGetDevice(&prev);
        if (prev == want)
            prev = -1;
        else
            (void)hipSetDevice(want);
    }
    ~DeviceGuard()
    {
        if (prev >= 0)
            (void)hipSetDevice(prev);
    }
};

// host staging memory that cannot throw across the C ABI: a failed allocation is reported as SCPP_E_HIP by the caller
template <class T>
struct HostBuf
{
    T *p;
    size_t n;
    explicit HostBuf(size_t n_) : p(static_cast<T *>(std::malloc((n_ ? n_ : 1) * sizeof(T)))), n(n_) {}
    ~HostBuf() { std::free(p); }
    HostBuf(const HostBuf &) = delete;
    HostBuf &operator=(const HostBuf &) = delete;
};

static bool allFinite(const double *v, size_t n)
{
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(v[i]))
            return false;
    return true;
}

// the affine sweep's share of the products: feedforward terms, and what scpp_hip_lqr_download_affine hands out
static void clearAffineProducts(scpp_hip_lqr_ctx *c)
{
    c->have_ff = c->have_affine = c->affine_kept = false;
}

// the products of a gain sweep, beyond the gains themselves
static void clearGainProducts(scpp_hip_lqr_ctx *c)
{
    c->have_p = c->have_disc = false;
    clearAffineProducts(c);
}

// the result of a covariance or moments sweep (have_mom is read together with have_cov only)
static void clearSweepResult(scpp_hip_lqr_ctx *c)
{
    c->have_cov = false;
}

// the result of a filter sweep
static void clearFilterResult(scpp_hip_lqr_ctx *c)
{
    c->have_filt = false;
}

// the gains changed: a filter result that carries the loop's covariance went with them
static void clearLoopFilterResult(scpp_hip_lqr_ctx *c)
{
    if (c->filt_loop)
        clearFilterResult(c);
}

// whatever changes the trajectories or replaces the gains: no gains, no P, no covariance
static void invalidateGains(scpp_hip_lqr_ctx *c)
{
    c->have_gains = c->gains_computed = false;
    clearGainProducts(c);
    clearSweepResult(c);
    clearLoopFilterResult(c);
}

// a change of weights or parameters: gains the library computed are stale, gains the caller supplied (scpp_hip_lqr_set_gains) stay
static void invalidateComputedGains(scpp_hip_lqr_ctx *c)
{
    if (c->gains_computed)
        invalidateGains(c);
}

// what every launch needs: trajectories, and parameter rows for one or for that number of trajectories
static int readyToLaunch(const scpp_hip_lqr_ctx *c)
{
    return c->have_traj && c->have_par && (c->par_rows == 1 || c->par_rows == c->B) ? SCPP_OK : SCPP_E_STATE;
}

// what became of a launch: `found` = the model has a plugin, so a kernel was enqueued
static int enqueued(bool found)
{
    if (!found)
        return SCPP_E_ARG;
    return hipGetLastError() == hipSuccess ? SCPP_OK : SCPP_E_HIP;
}

// launch(Plugin{}) enqueues the kernel of the context's model
template <class F>
static int launchKernel(scpp_hip_lqr_ctx *c, F &&launch)
{
    return enqueued(withLqrPlugin(c->model, launch));
}

// *n_ok = the entries of the device array `status` [n] equal to SCPP_LQR_OK (n_ok == nullptr: nothing is downloaded)
static int countOk(scpp_hip_lqr_ctx *c, const int *status, size_t n, int *n_ok)
{
    if (!n_ok)
        return SCPP_OK;
    HostBuf<int> st(n);
    if (!st.p)
        return SCPP_E_HIP;
    CHECK_HIP(hipMemcpyAsync(st.p, status, n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    CHECK_HIP(hipStreamSynchronize(c->stream));
    int ok = 0;
    for (size_t i = 0; i < n; i++)
        ok += (st.p[i] == SCPP_LQR_OK);
    *n_ok = ok;
    return SCPP_OK;
}

// *buf holds at least `need` doubles afterwards; on failure *buf == nullptr and *cap == 0
static int growTo(scpp_hip_lqr_ctx *c, double **buf, size_t *cap, size_t need)
{
    if (need <= *cap)
        return SCPP_OK;
    CHECK_HIP(hipStreamSynchronize(c->stream));
    if (*buf)
        (void)hipFree(*buf);
    *buf = nullptr;
    *cap = 0;
    if (devAlloc(buf, need))
        return SCPP_E_HIP;
    *cap = need;
    return SCPP_OK;
}

// the per-flight buffers hold at least F flights afterwards; they only ever grow.  On failure they are gone and fl_cap == 0.
static int growFlights(scpp_hip_lqr_ctx *c, size_t F)
{
    if (F <= c->fl_cap)
        return SCPP_OK;
    CHECK_HIP(hipStreamSynchronize(c->stream));
    void *old[] = {c->xs, c->ox, c->ou, c->os, c->oi, c->onsat, c->oclip};
    for (void *p : old)
        if (p)
            (void)hipFree(p);
    c->xs = c->ox = c->ou = c->os = c->oclip = nullptr;
    c->oi = c->onsat = nullptr;
    c->fl_cap = 0;
    c->have_track = false; // the results of the last flights went with the buffers
    if (devAlloc(&c->xs, F * c->nx) | devAlloc(&c->ox, F * c->nx) | devAlloc(&c->ou, F * c->nu) | devAlloc(&c->os, F * 4) | devAlloc(&c->oi, F * 2) |
        devAlloc(&c->onsat, F) | devAlloc(&c->oclip, F))
        return SCPP_E_HIP;
    c->fl_cap = F;
    return SCPP_OK;
}

// a group of buffers that are allocated by the first call that needs them and live as long as the context
struct OwnedBuffer
{
    double **buf;
    size_t n;
};

// every buffer of the group is allocated afterwards; nothing happens when all are.  A failed allocation frees the whole group, so a later
// call starts over and no launch ever sees some of them.
static int allocateTogether(std::initializer_list<OwnedBuffer> group)
{
    bool all = true;
    for (const OwnedBuffer &b : group)
        all = all && *b.buf;
    if (all)
        return SCPP_OK;
    int rc = 0;
    for (const OwnedBuffer &b : group)
        if (!*b.buf)
            rc |= devAlloc(b.buf, b.n);
    if (!rc)
        return SCPP_OK;
    for (const OwnedBuffer &b : group)
    {
        if (*b.buf)
            (void)hipFree(*b.buf);
        *b.buf = nullptr;
    }
    return SCPP_E_HIP;
}

// a buffer a sweep fills on request: `need` doubles (0: not asked for)
struct KeepBuffer
{
    double **buf;
    size_t *cap;
    size_t need;
};

// One gain sweep (Riccati, affine, discrete), c != nullptr.  The order is the ABI's: a failed growTo leaves the products cleared and have_gains
// as it was.  launch() enqueues the kernel and returns its code; kept() sets the flags of what this sweep keeps.
template <class Launch, class Kept>
static int runGainSweep(scpp_hip_lqr_ctx *c, int steps, int *n_ok, std::initializer_list<KeepBuffer> buffers, Launch &&launch, Kept &&kept)
{
    if (steps < 1)
        return SCPP_E_ARG;
    if (int rc = readyToLaunch(c))
        return rc;
    if (long(c->K - 1) * steps > 0x7fffffffL)
        return SCPP_E_ARG; // the step count behind node 0 is reported as an int32
    DeviceGuard guard(c->device);
    clearGainProducts(c);
    for (const KeepBuffer &k : buffers)
        if (int rc = growTo(c, k.buf, k.cap, k.need))
            return rc;
    if (int rc = launch())
        return rc;
    c->have_gains = c->gains_computed = true;
    kept();
    clearSweepResult(c);
    clearLoopFilterResult(c);
    return countOk(c, c->gstatus, size_t(c->B) * c->K, n_ok);
}

// what the moments sweep takes beyond the covariance sweep's arguments
struct MomentsRequest
{
    int feedforward;
    const double *mean0;
    int rows;
};

// one forward sweep per trajectory: the continuous loop's covariance (lqr_covariance_kernel), with `discrete` the node-rate hold's
// (lqr_covariance_discrete_kernel), with `mom` the continuous loop's covariance and mean (lqr_moments_kernel); all three take the covariance
// inputs and leave the covariance in the same buffers
static int propagateCovariance(scpp_hip_lqr_ctx *c, int steps, int keep_cov, int *n_ok, bool discrete, const MomentsRequest *mom = nullptr)
{
    if (!c || steps < 1 || (mom && mom->feedforward != 0 && mom->feedforward != 1))
        return SCPP_E_ARG;
    if (int rc = readyToLaunch(c))
        return rc;
    if (mom && mom->mean0 && ((mom->rows != 1 && mom->rows != c->B) || !allFinite(mom->mean0, size_t(mom->rows) * c->nx)))
        return SCPP_E_ARG;
    if (!c->have_gains || !c->have_cov_in || (c->s0_rows != 1 && c->s0_rows != c->B) || (mom && mom->feedforward && !c->have_ff))
        return SCPP_E_STATE; // no gains, no initial covariance, one for another number of trajectories, or no feedforward term to add
    DeviceGuard guard(c->device);
    const size_t Bm = size_t(c->Bmax), K = size_t(c->K), nx = size_t(c->nx), nu = size_t(c->nu);
    clearSweepResult(c);
    c->have_mom = false;
    if (mom && !c->m0 && (devAlloc(&c->m0, Bm * nx) | devAlloc(&c->cmean, Bm * K * nx) | devAlloc(&c->cdu, Bm * K * nu)))
        return SCPP_E_HIP;
    if (keep_cov)
        if (int rc = growTo(c, &c->cov, &c->cov_cap, size_t(c->B) * K * nx * nx))
            return rc;
    if (mom && mom->mean0)
    {
        CHECK_HIP(hipMemcpyAsync(c->m0, mom->mean0, size_t(mom->rows) * nx * sizeof(double), hipMemcpyHostToDevice, c->stream));
        CHECK_HIP(hipStreamSynchronize(c->stream)); // the host array is the caller's
    }
    const int *gstatus = c->gains_computed ? c->gstatus : nullptr;
    const int s0_stride = c->s0_rows == 1 ? 0 : c->nx * c->nx;
    double *cov = keep_cov ? c->cov : nullptr;
    int rc;
    if (mom)
        rc = enqueued(launchMomentsSweep(c->model, c->stream, c->B, c->K, c->nU, c->uRows, steps, c->tX, c->tU, c->tT, c->par, c->par_stride, c->G,
                                         gstatus, c->s0, s0_stride, c->cw, mom->feedforward ? c->ff : nullptr, mom->mean0 ? c->m0 : nullptr,
                                         mom->rows == 1 ? 0 : c->nx, c->cstd, c->cin, c->cfin, c->cstatus, cov, c->cmean, c->cdu));
    else
        rc = launchKernel(c, [&](auto pl) {
            using P = decltype(pl);
            auto go = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, dim3(unsigned(c->B)), dim3(WAVE), 0, c->stream, c->K, c->nU, c->uRows, steps, c->tX, c->tU, c->tT,
                                   (const double *)c->par, c->par_stride, (const double *)c->G, gstatus, (const double *)c->s0, s0_stride,
                                   (const double *)c->cw, c->cstd, c->cin, c->cfin, c->cstatus, cov);
            };
            if (discrete)
                go(lqr_covariance_discrete_kernel<P>);
            else
                go(lqr_covariance_kernel<P>);
        });
    if (rc)
        return rc;
    c->have_cov = true;
    c->have_mom = mom != nullptr;
    c->cov_kept = keep_cov != 0;
    return countOk(c, c->cstatus, size_t(c->B), n_ok);
}

extern "C"
{

const char *scpp_hip_lqr_version(void)
{
#ifdef SCPP_HIP_EMU
    return "scpp_hip_lqr 2 (cpu emulation)";
#else
    return "scpp_hip_lqr 2 (gfx950)";
#endif
}

int scpp_hip_lqr_create(scpp_hip_lqr_ctx **out, int device_id, int model_id, int K, int batch_max, int foh)
{
    if (!out || K < 2 || batch_max < 1)
        return SCPP_E_ARG;
    *out = nullptr;
    if (!withLqrPlugin(model_id, [](auto) {}))
        return SCPP_E_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev)
        return SCPP_E_HIP;
    DeviceGuard guard(device_id);
    scpp_hip_lqr_ctx *c = new (std::nothrow) scpp_hip_lqr_ctx;
    if (!c)
        return SCPP_E_HIP;
    c->device = device_id;
    c->model = model_id;
    c->K = K;
    c->nU = foh ? K : K - 1;
    c->Bmax = batch_max;
    (void)withLqrPlugin(model_id, [&](auto pl) {
        using P = decltype(pl);
        c->nx = P::Model::NX;
        c->nu = P::Model::NU;
        c->np = P::Model::NP;
        c->nr = P::NR;
    });
    if (hipStreamCreate(&c->stream) != hipSuccess)
    {
        delete c;
        return SCPP_E_HIP;
    }
    const size_t B = size_t(batch_max), nx = size_t(c->nx), nu = size_t(c->nu);
    int rc = 0;
    rc |= devAlloc(&c->X, B * K * nx);
    rc |= devAlloc(&c->U, B * c->nU * nu);
    rc |= devAlloc(&c->T, B);
    rc |= devAlloc(&c->par, B * c->np);
    rc |= devAlloc(&c->q, nx);
    rc |= devAlloc(&c->r, nu);
    rc |= devAlloc(&c->qf, nx);
    rc |= devAlloc(&c->G, B * K * nu * nx);
    rc |= devAlloc(&c->gstatus, B * K);
    rc |= devAlloc(&c->giters, B * K);
    rc |= devAlloc(&c->xs, B * nx);
    rc |= devAlloc(&c->xf, nx);
    rc |= devAlloc(&c->ox, B * nx);
    rc |= devAlloc(&c->ou, B * nu);
    rc |= devAlloc(&c->os, B * 4);
    rc |= devAlloc(&c->oi, B * 2);
    rc |= devAlloc(&c->onsat, B);
    rc |= devAlloc(&c->oclip, B);
    c->fl_cap = B;
    if (rc == 0)
    {
        HostBuf<double> one(nx > nu ? nx : nu);
        rc |= one.p == nullptr;
        for (size_t i = 0; one.p && i < one.n; i++)
            one.p[i] = 1.;
        rc |= rc || hipMemcpy(c->q, one.p, nx * sizeof(double), hipMemcpyHostToDevice) != hipSuccess;
        rc |= rc || hipMemcpy(c->r, one.p, nu * sizeof(double), hipMemcpyHostToDevice) != hipSuccess;
    }
    if (rc)
    {
        scpp_hip_lqr_destroy(c);
        return SCPP_E_HIP;
    }
    *out = c;
    return SCPP_OK;
}

int scpp_hip_lqr_destroy(scpp_hip_lqr_ctx *c)
{
    if (!c)
        return SCPP_E_ARG;
    DeviceGuard guard(c->device);
    if (c->stream)
        (void)hipStreamSynchronize(c->stream);
    void *bufs[] = {c->X, c->U, c->T, c->par, c->q, c->r, c->qf, c->P, c->G, c->gstatus, c->giters, c->xs, c->xf, c->ox, c->ou, c->os, c->oi, c->rx, c->ru, c->rt, c->rn,
                    c->s0, c->cw, c->cstd, c->cin, c->cfin, c->cov, c->cstatus, c->onsat, c->oclip, c->lim, c->phi, c->gam, c->ff, c->ap, c->as, c->m0, c->cmean, c->cdu, c->nsd,
                    c->mH, c->mv, c->fL, c->fes, c->ffe, c->fec, c->fss, c->fic, c->ffs, c->fxc, c->fstatus};
    for (void *p : bufs)
        if (p)
            (void)hipFree(p);
    if (c->stream)
        (void)hipStreamDestroy(c->stream);
    delete c;
    return SCPP_OK;
}

int scpp_hip_lqr_dims(scpp_hip_lqr_ctx *c, int *nx, int *nu, int *np, int *nr)
{
    if (!c)
        return SCPP_E_ARG;
    if (nx)
        *nx = c->nx;
    if (nu)
        *nu = c->nu;
    if (np)
        *np = c->np;
    if (nr)
        *nr = c->nr;
    return SCPP_OK;
}

int scpp_hip_lqr_set_weights(scpp_hip_lqr_ctx *c, const double *q, const double *r)
{
    if (!c || !q || !r)
        return SCPP_E_ARG;
    for (int i = 0; i < c->nx; i++)
        if (!std::isfinite(q[i]) || !(q[i] > 0.))
            return SCPP_E_ARG;
    for (int i = 0; i < c->nu; i++)
        if (!std::isfinite(r[i]) || !(r[i] > 0.))
            return SCPP_E_ARG;
    DeviceGuard guard(c->device);
    CHECK_HIP(hipMemcpyAsync(c->q, q, size_t(c->nx) * sizeof(double), hipMemcpyHostToDevice, c->stream));
    CHECK_HIP(hipMemcpyAsync(c->r, r, size_t(c->nu) * sizeof(double), hipMemcpyHostToDevice, c->stream));
    CHECK_HIP(hipStreamSynchronize(c->stream)); // the host arrays are the caller's
    invalidateComputedGains(c);
    return SCPP_OK;
}

int scpp_hip_lqr_set_flow_params(scpp_hip_lqr_ctx *c, const double *par, int B)
{
    if (!c || !par || B < 1 || B > c->Bmax)
        return SCPP_E_ARG;
    DeviceGuard guard(c->device);
    CHECK_HIP(hipMemcpyAsync(c->par, par, size_t(B) * c->np * sizeof(double), hipMemcpyHostToDevice, c->stream));
    CHECK_HIP(hipStreamSynchronize(c->stream));
    c->par_stride = (B == 1) ? 0 : c->np;
    c->par_rows = B;
    c->have_par = true;
    clearSweepResult(c);
    clearFilterResult(c);
    clearAffineProducts(c); // the defect of the nominal is one of THIS plant
    invalidateComputedGains(c);
    return SCPP_OK;
}

int scpp_hip_lqr_set_trajectories(scpp_hip_lqr_ctx *c, const double *X, const double *U, const double *t, int B)
{
    if (!c || !X || !U || !t || B < 1 || B > c->Bmax)
        return SCPP_E_ARG;
    DeviceGuard guard(c->device);
    CHECK_HIP(hipMemcpyAsync(c->X, X, size_t(B) * c->K * c->nx * sizeof(double), hipMemcpyHostToDevice, c->stream));
    CHECK_HIP(hipMemcpyAsync(c->U, U, size_t(B) * c->nU * c->nu * sizeof(double), hipMemcpyHostToDevice, c->stream));
    CHECK_HIP(hipMemcpyAsync(c->T, t, size_t(B) * sizeof(double), hipMemcpyHostToDevice, c->stream));
    CHECK_HIP(hipStreamSynchronize(c->stream));
    c->tX = c->X;
    c->tU = c->U;
    c->tT = c->T;
    c->uRows = c->nU;
    c->B = B;
    c->have_traj = true;
    invalidateGains(c);
    clearFilterResult(c);
    return SCPP_OK;
}

int scpp_hip_lqr_set_trajectories_device(scpp_hip_lqr_ctx *c, const void *dX, const void *dU, const void *dt, int B, int u_rows)
{
    if (!c || !dX || !dU || !dt || B < 1 || B > c->Bmax || u_rows < c->nU)
        return SCPP_E_ARG;
    c->tX = static_cast<const double *>(dX);
    c->tU = static_cast<const double *>(dU);
    c->tT = static_cast<const double *>(dt);
    c->uRows = u_rows;
    c->B = B;
    c->have_traj = true;
    invalidateGains(c);
    clearFilterResult(c);
    return SCPP_OK;
}

int scpp_hip_lqr_compute_gains(scpp_hip_lqr_ctx *c, int *n_ok)
{
    if (!c)
        return SCPP_E_ARG;
    if (int rc = readyToLaunch(c))
        return rc;
    DeviceGuard guard(c->device);
    const long nodes = long(c->B) * c->K;
    const unsigned grid = unsigned((nodes + 1) / 2);
    int rc = launchKernel(c, [&](auto pl) {
        using P = decltype(pl);
        hipLaunchKernelGGL((lqr_gain_kernel<P>), dim3(grid), dim3(WAVE), 0, c->stream, nodes, c->K, c->nU, c->uRows, c->tX, c->tU,
                           (const double *)c->par, c->par_stride, (const double *)c->q, (const double *)c->r, c->G, c->gstatus, c->giters);
    });
    if (rc)
        return rc;
    c->have_gains = c->gains_computed = true;
    clearGainProducts(c);
    clearSweepResult(c);
    clearLoopFilterResult(c);
    return countOk(c, c->gstatus, size_t(nodes), n_ok);
}

int scpp_hip_lqr_set_terminal_weights(scpp_hip_lqr_ctx *c, const double *qf)
{
    if (!c)
        return SCPP_E_ARG;
    if (qf)
    {
        for (int i = 0; i < c->nx; i++)
            if (!std::isfinite(qf[i]) || !(qf[i] > 0.))
                return SCPP_E_ARG;
        DeviceGuard guard(c->device);
        CHECK_HIP(hipMemcpyAsync(c->qf, qf, size_t(c->nx) * sizeof(double), hipMemcpyHostToDevice, c->stream));
        CHECK_HIP(hipStreamSynchronize(c->stream));
    }
    c->have_qf = qf != nullptr;
    invalidateComputedGains(c);
    return SCPP_OK;
}

int scpp_hip_lqr_compute_gains_riccati(scpp_hip_lqr_ctx *c, int steps, int keep_p, int *n_ok)
{
    if (!c)
        return SCPP_E_ARG;
    const size_t nodes = size_t(c->B) * c->K;
    return runGainSweep(
        c, steps, n_ok, {{&c->P, &c->P_cap, keep_p ? nodes * c->nx * c->nx : 0}},
        [&] {
            return launchKernel(c, [&](auto pl) {
                using P = decltype(pl);
                hipLaunchKernelGGL((lqr_riccati_kernel<P>), dim3(unsigned(c->B)), dim3(WAVE), 0, c->stream, c->K, c->nU, c->uRows, steps, c->tX, c->tU,
                                   c->tT, (const double *)c->par, c->par_stride, (const double *)c->q, (const double *)c->r,
                                   (const double *)(c->have_qf ? c->qf : c->q), c->G, c->gstatus, c->giters, keep_p ? c->P : (double *)nullptr);
            });
        },
        [&] { c->have_p = keep_p != 0; });
}

int scpp_hip_lqr_download_riccati(scpp_hip_lqr_ctx *c, double *P)
{
    if (!c || !P)
        return SCPP_E_ARG;
    if (!c->have_p)
        return SCPP_E_STATE;
    DeviceGuard guard(c->device);
    CHECK_HIP(hipMemcpyAsync(P, c->P, size_t(c->B) * c->K * c->nx * c->nx * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    CHECK_HIP(hipStreamSynchronize(c->stream));
    return SCPP_OK;
}

int scpp_hip_lqr_compute_gains_affine(scpp_hip_lqr_ctx *c, int steps, int keep, int *n_ok)
{
    if (!c)
        return SCPP_E_ARG;
    const size_t nodes = size_t(c->B) * c->K, kept = keep ? nodes : 0;
    return runGainSweep(
        c, steps, n_ok,
        {{&c->ff, &c->ff_cap, size_t(c->Bmax) * c->K * c->nu}, {&c->P, &c->P_cap, kept * c->nx * c->nx}, {&c->ap, &c->ap_cap, kept * c->nx},
         {&c->as, &c->as_cap, kept}},
        [&] {
            return enqueued(launchAffineSweep(c->model, c->stream, c->B, c->K, c->nU, c->uRows, steps, c->tX, c->tU, c->tT, c->par, c->par_stride, c->q,
                                              c->r, c->have_qf ? c->qf : c->q, c->G, c->gstatus, c->giters, c->ff, keep ? c->P : nullptr,
                                              keep ? c->ap : nullptr, keep ? c->as : nullptr));
        },
        [&] {
            c->have_affine = c->have_ff = true;
            c->affine_kept = keep != 0;
        });
}

int scpp_hip_lqr_download_affine(scpp_hip_lqr_ctx *c, double *ff, double *P, double *p, double *s)
{
    if (!c)
        return SCPP_E_ARG;
    if (!c->have_affine || ((P || p || s) && !c->affine_kept))
        return SCPP_E_STATE;
    DeviceGuard guard(c->device);
    const size_t nodes = size_t(c->B) * c->K, nx = size_t(c->nx);
    if (ff)
        CHECK_HIP(hipMemcpyAsync(ff, c->ff, nodes * c->nu * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (P)
        CHECK_HIP(hipMemcpyAsync(P, c->P, nodes * nx * nx * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (p)
        CHECK_HIP(hipMemcpyAsync(p, c->ap, nodes * nx * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (s)
        CHECK_HIP(hipMemcpyAsync(s, c->as, nodes * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    CHECK_HIP(hipStreamSynchronize(c->stream));
    return SCPP_OK;
}

int scpp_hip_lqr_set_feedforward_terms(scpp_hip_lqr_ctx *c, const double *ff)
{
    if (!c || !ff)
        return SCPP_E_ARG;
    if (!c->have_gains)
        return SCPP_E_STATE;
    const size_t n = size_t(c->B) * c->K * c->nu;
    if (!allFinite(ff, n))
        return SCPP_E_ARG;
    DeviceGuard guard(c->device);
    if (int rc = growTo(c, &c->ff, &c->ff_cap, size_t(c->Bmax) * c->K * c->nu))
        return rc;
    CHECK_HIP(hipMemcpyAsync(c->ff, ff, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    CHECK_HIP(hipStreamSynchronize(c->stream));
    c->have_ff = true;
    c->have_affine = c->affine_kept = false; // the terms are the caller's now: scpp_hip_lqr_download_affine has nothing of its own left
    return SCPP_OK;
}

int scpp_hip_lqr_set_feedforward(scpp_hip_lqr_ctx *c, int mode)
{
    if (!c || (mode != 0 && mode != 1))
        return SCPP_E_ARG;
    c->ffmode = mode;
    return SCPP_OK;
}

int scpp_hip_lqr_compute_gains_discrete(scpp_hip_lqr_ctx *c, int steps, int keep, int *n_ok)
{
    if (!c)
        return SCPP_E_ARG;
    const size_t nodes = keep ? size_t(c->B) * c->K : 0, segs = keep ? size_t(c->B) * (c->K - 1) : 0;
    return runGainSweep(
        c, steps, n_ok,
        {{&c->P, &c->P_cap, nodes * c->nx * c->nx}, {&c->phi, &c->phi_cap, segs * c->nx * c->nx}, {&c->gam, &c->gam_cap, segs * c->nx * c->nu}},
        [&] {
            return launchKernel(c, [&](auto pl) {
                using P = decltype(pl);
                hipLaunchKernelGGL((lqr_discrete_kernel<P>), dim3(unsigned(c->B)), dim3(WAVE), 0, c->stream, c->K, c->nU, c->uRows, steps, c->tX, c->tU,
                                   c->tT, (const double *)c->par, c->par_stride, (const double *)c->q, (const double *)c->r,
                                   (const double *)(c->have_qf ? c->qf : c->q), c->G, c->gstatus, c->giters, keep ? c->P : (double *)nullptr,
                                   keep ? c->phi : (double *)nullptr, keep ? c->gam : (double *)nullptr);
            });
        },
        [&] { c->have_disc = keep != 0; });
}

int scpp_hip_lqr_download_discrete(scpp_hip_lqr_ctx *c, double *P, double *Phi, double *Gamma)
{
    if (!c)
        return SCPP_E_ARG;
    if (!c->have_disc)
        return SCPP_E_STATE;
    DeviceGuard guard(c->device);
    const size_t B = size_t(c->B), K = size_t(c->K), nx = size_t(c->nx), nu = size_t(c->nu);
    if (P)
        CHECK_HIP(hipMemcpyAsync(P, c->P, B * K * nx * nx * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (Phi)
        CHECK_HIP(hipMemcpyAsync(Phi, c->phi, B * (K - 1) * nx * nx * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (Gamma)
        CHECK_HIP(hipMemcpyAsync(Gamma, c->gam, B * (K - 1) * nx * nu * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    CHECK_HIP(hipStreamSynchronize(c->stream));
    return SCPP_OK;
}

int scpp_hip_lqr_set_feedback_hold(scpp_hip_lqr_ctx *c, int mode)
{
    if (!c || (mode != 0 && mode != 1))
        return SCPP_E_ARG;
    c->hold = mode;
    return SCPP_OK;
}

int scpp_hip_lqr_download_gains(scpp_hip_lqr_ctx *c, double *gains, int *status, int *iters)
{
    if (!c)
        return SCPP_E_ARG;
    if (!c->have_gains)
        return SCPP_E_STATE;
    if ((status || iters) && !c->gains_computed)
        return SCPP_E_STATE; // user-supplied gains carry no status
    DeviceGuard guard(c->device);
    const size_t nodes = size_t(c->B) * c->K;
    if (gains)
        CHECK_HIP(hipMemcpyAsync(gains, c->G, nodes * c->nu * c->nx * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (status)
        CHECK_HIP(hipMemcpyAsync(status, c->gstatus, nodes * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (iters)
        CHECK_HIP(hipMemcpyAsync(iters, c->giters, nodes * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    CHECK_HIP(hipStreamSynchronize(c->stream));
    return SCPP_OK;
}

int scpp_hip_lqr_set_gains(scpp_hip_lqr_ctx *c, const double *gains)
{
    if (!c || !gains)
        return SCPP_E_ARG;
    if (!c->have_traj)
        return SCPP_E_STATE;
    const size_t n = size_t(c->B) * c->K * c->nu * c->nx;
    if (!allFinite(gains, n))
        return SCPP_E_ARG;
    DeviceGuard guard(c->device);
    CHECK_HIP(hipMemcpyAsync(c->G, gains, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    CHECK_HIP(hipStreamSynchronize(c->stream));
    invalidateGains(c);
    c->have_gains = true;
    return SCPP_OK;
}

int scpp_hip_lqr_set_covariance_inputs(scpp_hip_lqr_ctx *c, const double *sigma0, int B, const double *w)
{
    if (!c || !sigma0)
        return SCPP_E_ARG;
    if (!c->have_traj)
        return SCPP_E_STATE; // B is judged against the number of trajectories
    if (B != 1 && B != c->B)
        return SCPP_E_ARG;
    const size_t nx = size_t(c->nx), nn = nx * nx;
    for (size_t b = 0; b < size_t(B); b++)
    {
        const double *s = sigma0 + b * nn;
        if (!allFinite(s, nn))
            return SCPP_E_ARG;
        for (size_t i = 0; i < nx; i++)
        {
            if (s[i * nx + i] < 0.)
                return SCPP_E_ARG;
            for (size_t j = 0; j < i; j++)
                if (s[i * nx + j] != s[j * nx + i])
                    return SCPP_E_ARG; // symmetric to the bit: the kernel reads one half for the other
        }
    }
    for (size_t i = 0; w && i < nx; i++)
        if (!std::isfinite(w[i]) || w[i] < 0.)
            return SCPP_E_ARG;
    DeviceGuard guard(c->device);
    if (!c->s0)
    {
        const size_t Bm = size_t(c->Bmax), nu = size_t(c->nu);
        int rc = devAlloc(&c->s0, Bm * nn) | devAlloc(&c->cw, nx) | devAlloc(&c->cstd, Bm * c->K * nx) | devAlloc(&c->cin, Bm * c->K * nu * nu) |
                 devAlloc(&c->cfin, Bm * nn) | devAlloc(&c->cstatus, Bm);
        if (rc)
            return SCPP_E_HIP;
    }
    HostBuf<double> zero(nx);
    if (!zero.p)
        return SCPP_E_HIP;
    for (size_t i = 0; i < nx; i++)
        zero.p[i] = 0.;
    CHECK_HIP(hipMemcpyAsync(c->s0, sigma0, size_t(B) * nn * sizeof(double), hipMemcpyHostToDevice, c->stream));
    CHECK_HIP(hipMemcpyAsync(c->cw, w ? w : zero.p, nx * sizeof(double), hipMemcpyHostToDevice, c->stream));
    CHECK_HIP(hipStreamSynchronize(c->stream)); // the host arrays are the caller's
    c->s0_rows = B;
    c->have_cov_in = true;
    clearSweepResult(c);
    clearFilterResult(c);
    return SCPP_OK;
}

int scpp_hip_lqr_set_measurement(scpp_hip_lqr_ctx *c, const double *H, int ny, const double *v)
{
    if (!c)
        return SCPP_E_ARG;
    if (!H)
    {
        c->have_meas = false;
        clearFilterResult(c);
        return SCPP_OK;
    }
    if (!v || ny < 1 || ny > RT || !allFinite(H, size_t(ny) * c->nx) || !allFinite(v, size_t(ny)))
        return SCPP_E_ARG;
    for (int m = 0; m < ny; m++)
        if (!(v[m] > 0.))
            return SCPP_E_ARG;
    DeviceGuard guard(c->device);
    if (int rc = allocateTogether({{&c->mH, size_t(RT) * c->nx}, {&c->mv, size_t(RT)}}))
        return rc;
    CHECK_HIP(hipMemcpyAsync(c->mH, H, size_t(ny) * c->nx * sizeof(double), hipMemcpyHostToDevice, c->stream));
    CHECK_HIP(hipMemcpyAsync(c->mv, v, size_t(ny) * sizeof(double), hipMemcpyHostToDevice, c->stream));
    CHECK_HIP(hipStreamSynchronize(c->stream)); // the host arrays are the caller's
    c->ny = ny;
    c->have_meas = true;
    clearFilterResult(c);
    return SCPP_OK;
}

int scpp_hip_lqr_filter(scpp_hip_lqr_ctx *c, int steps, int closed_loop, int keep, int *n_ok)
{
    if (!c || steps < 1)
        return SCPP_E_ARG;
    if (int rc = readyToLaunch(c))
        return rc;
    if (!c->have_cov_in || (c->s0_rows != 1 && c->s0_rows != c->B) || !c->have_meas || (closed_loop && !c->have_gains))
        return SCPP_E_STATE; // no initial covariance, one for another number of trajectories, no measurement, or no gains to close the loop with
    DeviceGuard guard(c->device);
    const size_t Bm = size_t(c->Bmax), K = size_t(c->K), nx = size_t(c->nx), nu = size_t(c->nu);
    clearFilterResult(c);
    if (int rc = allocateTogether({{&c->fL, Bm * K * nx * RT}, {&c->fes, Bm * K * nx}, {&c->ffe, Bm * nx * nx}}))
        return rc;
    if (!c->fstatus && devAlloc(&c->fstatus, Bm))
    {
        c->fstatus = nullptr;
        return SCPP_E_HIP;
    }
    if (closed_loop)
        if (int rc = allocateTogether({{&c->fss, Bm * K * nx}, {&c->fic, Bm * K * nu * nu}, {&c->ffs, Bm * nx * nx}}))
            return rc;
    if (keep)
    {
        if (int rc = growTo(c, &c->fec, &c->fec_cap, size_t(c->B) * K * nx * nx))
            return rc;
        if (closed_loop)
            if (int rc = growTo(c, &c->fxc, &c->fxc_cap, size_t(c->B) * K * nx * nx))
                return rc;
    }
    const int *gstatus = (closed_loop && c->gains_computed) ? c->gstatus : nullptr;
    const int s0_stride = c->s0_rows == 1 ? 0 : c->nx * c->nx;
    if (int rc = enqueued(launchFilterSweep(c->model, c->stream, closed_loop != 0, c->B, c->K, c->nU, c->uRows, steps, c->tX, c->tU, c->tT, c->par,
                                            c->par_stride, c->G, gstatus, c->s0, s0_stride, c->cw, c->mH, c->mv, c->ny, c->fL, c->fes, c->ffe,
                                            c->fstatus, keep ? c->fec : nullptr, c->fss, c->fic, c->ffs, (keep && closed_loop) ? c->fxc : nullptr)))
        return rc;
    c->have_filt = true;
    c->filt_loop = closed_loop != 0;
    c->filt_kept = keep != 0;
    return countOk(c, c->fstatus, size_t(c->B), n_ok);
}

int scpp_hip_lqr_download_filter(scpp_hip_lqr_ctx *c, double *L, double *error_std, double *final_error_cov, int *status, double *error_cov,
                                 double *state_std, double *input_cov, double *final_state_cov, double *estimate_cov)
{
    if (!c)
        return SCPP_E_ARG;
    if (!c->have_filt || ((error_cov || estimate_cov) && !c->filt_kept) || ((state_std || input_cov || final_state_cov || estimate_cov) && !c->filt_loop))
        return SCPP_E_STATE;
    DeviceGuard guard(c->device);
    const size_t B = size_t(c->B), K = size_t(c->K), nx = size_t(c->nx), nu = size_t(c->nu);
    const struct
    {
        void *dst;
        const void *src;
        size_t bytes;
    } copies[] = {{L, c->fL, B * K * nx * size_t(c->ny) * sizeof(double)},
                  {error_std, c->fes, B * K * nx * sizeof(double)},
                  {final_error_cov, c->ffe, B * nx * nx * sizeof(double)},
                  {status, c->fstatus, B * sizeof(int)},
                  {error_cov, c->fec, B * K * nx * nx * sizeof(double)},
                  {state_std, c->fss, B * K * nx * sizeof(double)},
                  {input_cov, c->fic, B * K * nu * nu * sizeof(double)},
                  {final_state_cov, c->ffs, B * nx * nx * sizeof(double)},
                  {estimate_cov, c->fxc, B * K * nx * nx * sizeof(double)}};
    for (const auto &cp : copies)
        if (cp.dst)
            CHECK_HIP(hipMemcpyAsync(cp.dst, cp.src, cp.bytes, hipMemcpyDeviceToHost, c->stream));
    CHECK_HIP(hipStreamSynchronize(c->stream));
    return SCPP_OK;
}

int scpp_hip_lqr_propagate_covariance(scpp_hip_lqr_ctx *c, int steps, int keep_cov, int *n_ok)
{
    return propagateCovariance(c, steps, keep_cov, n_ok, false);
}

int scpp_hip_lqr_propagate_covariance_discrete(scpp_hip_lqr_ctx *c, int steps, int keep_cov, int *n_ok)
{
    return propagateCovariance(c, steps, keep_cov, n_ok, true);
}

int scpp_hip_lqr_propagate_moments(scpp_hip_lqr_ctx *c, int steps, int keep_cov, int feedforward, const double *mean0, int rows, int *n_ok)
{
    const MomentsRequest mom = {feedforward, mean0, rows};
    return propagateCovariance(c, steps, keep_cov, n_ok, false, &mom);
}

int scpp_hip_lqr_download_moments(scpp_hip_lqr_ctx *c, double *mean, double *input_mean)
{
    if (!c)
        return SCPP_E_ARG;
    if (!c->have_cov || !c->have_mom)
        return SCPP_E_STATE;
    DeviceGuard guard(c->device);
    const size_t nodes = size_t(c->B) * c->K;
    if (mean)
        CHECK_HIP(hipMemcpyAsync(mean, c->cmean, nodes * c->nx * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (input_mean)
        CHECK_HIP(hipMemcpyAsync(input_mean, c->cdu, nodes * c->nu * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    CHECK_HIP(hipStreamSynchronize(c->stream));
    return SCPP_OK;
}

int scpp_hip_lqr_download_covariance(scpp_hip_lqr_ctx *c, double *state_std, double *input_cov, double *final_cov, int *status, double *cov)
{
    if (!c)
        return SCPP_E_ARG;
    if (!c->have_cov || (cov && !c->cov_kept))
        return SCPP_E_STATE;
    DeviceGuard guard(c->device);
    const size_t B = size_t(c->B), K = size_t(c->K), nx = size_t(c->nx), nu = size_t(c->nu);
    if (state_std)
        CHECK_HIP(hipMemcpyAsync(state_std, c->cstd, B * K * nx * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (input_cov)
        CHECK_HIP(hipMemcpyAsync(input_cov, c->cin, B * K * nu * nu * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (final_cov)
        CHECK_HIP(hipMemcpyAsync(final_cov, c->cfin, B * nx * nx * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (status)
        CHECK_HIP(hipMemcpyAsync(status, c->cstatus, B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (cov)
        CHECK_HIP(hipMemcpyAsync(cov, c->cov, B * K * nx * nx * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    CHECK_HIP(hipStreamSynchronize(c->stream));
    return SCPP_OK;
}

int scpp_hip_lqr_set_input_limits(scpp_hip_lqr_ctx *c, const double *lim, int B)
{
    if (!c)
        return SCPP_E_ARG;
    if (!lim)
    {
        c->have_lim = false;
        return SCPP_OK;
    }
    if (B < 1 || B > c->Bmax)
        return SCPP_E_ARG;
    bool thrust_vector = false;
    (void)withLqrPlugin(c->model, [&](auto pl) {
        thrust_vector = decltype(pl)::THRUST_VECTOR;
    });
    HostBuf<double> rows(size_t(B) * LIM_ROW);
    if (!rows.p)
        return SCPP_E_HIP;
    for (int b = 0; b < B; b++)
    {
        const double t_min = lim[b * 3 + 0], t_max = lim[b * 3 + 1], angle = lim[b * 3 + 2];
        if (!allFinite(lim + b * 3, 3) || t_min < 0. || !(t_max > t_min) || !(angle > 0.) || !(angle < 1.5707963267948966))
            return SCPP_E_ARG;
        if (thrust_vector && t_min > t_max * std::cos(angle))
            return SCPP_E_ARG; // the three steps end inside the set only under this condition: the T_max scaling could undo the T_min floor
        double *r = rows.p + size_t(b) * LIM_ROW;
        r[0] = t_min;
        r[1] = t_max;
        r[2] = angle;
        r[3] = std::tan(angle);
    }
    DeviceGuard guard(c->device);
    if (!c->lim && devAlloc(&c->lim, size_t(c->Bmax) * LIM_ROW))
        return SCPP_E_HIP;
    CHECK_HIP(hipMemcpyAsync(c->lim, rows.p, rows.n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    CHECK_HIP(hipStreamSynchronize(c->stream));
    c->lim_rows = B;
    c->have_lim = true;
    return SCPP_OK;
}

int scpp_hip_lqr_set_disturbance(scpp_hip_lqr_ctx *c, const double *w, unsigned long long seed, unsigned long long flight_offset)
{
    if (!c)
        return SCPP_E_ARG;
    if (!w)
    {
        c->have_noise = false;
        return SCPP_OK;
    }
    if (c->nx > scpp_hip_lqr_ctx::NOISE_MAX_NX)
        return SCPP_E_UNSUPPORTED;
    for (int i = 0; i < c->nx; i++)
        if (!std::isfinite(w[i]) || w[i] < 0.)
            return SCPP_E_ARG;
    DeviceGuard guard(c->device);
    if (!c->nsd && devAlloc(&c->nsd, size_t(c->nx)))
        return SCPP_E_HIP;
    for (int i = 0; i < c->nx; i++)
        c->noise_w[i] = w[i];
    c->noise_seed = seed;
    c->noise_offset = flight_offset;
    c->have_noise = true;
    return SCPP_OK;
}

int scpp_hip_lqr_disturbance_normals(scpp_hip_lqr_ctx *c, unsigned long long seed, unsigned long long flight0, int flights, int step0, int steps,
                                     double *z)
{
    if (!c || flights < 1 || steps < 1 || step0 < 0 || !z)
        return SCPP_E_ARG;
    const size_t items = size_t(flights) * size_t(steps), n = items * size_t(c->nx);
    const size_t blocks = (items + WAVE - 1) / WAVE;
    if (blocks > 0x7fffffffu)
        return SCPP_E_ARG;
    DeviceGuard guard(c->device);
    double *dz = nullptr;
    if (devAlloc(&dz, n))
        return SCPP_E_HIP;
    int rc = launchKernel(c, [&](auto pl) {
        hipLaunchKernelGGL((lqr_noise_kernel<decltype(pl)::Model::NX>), dim3(unsigned(blocks)), dim3(WAVE), 0, c->stream, seed, flight0, long(flights),
                           unsigned(step0), steps, dz);
    });
    if (rc == SCPP_OK && hipMemcpyAsync(z, dz, n * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        rc = SCPP_E_HIP;
    if (hipStreamSynchronize(c->stream) != hipSuccess)
        rc = SCPP_E_HIP;
    (void)hipFree(dz);
    return rc;
}

int scpp_hip_lqr_set_stop_tolerance(scpp_hip_lqr_ctx *c, double stop_tol)
{
    if (!c || !(stop_tol >= 0.) || !std::isfinite(stop_tol))
        return SCPP_E_ARG;
    c->stop_tol = stop_tol;
    return SCPP_OK;
}

int scpp_hip_lqr_track(scpp_hip_lqr_ctx *c, const double *x_start, const double *x_final, int B, double time_step, int substeps, int max_steps,
                       int n_record, int write_steps, int *n_finite)
{
    return scpp_hip_lqr_track_samples(c, x_start, x_final, B, 1, time_step, substeps, max_steps, n_record, write_steps, n_finite);
}

int scpp_hip_lqr_track_samples(scpp_hip_lqr_ctx *c, const double *x_start, const double *x_final, int Btraj, int samples, double time_step,
                               int substeps, int max_steps, int n_record, int write_steps, int *n_finite)
{
    if (!c || !x_start || !x_final || Btraj < 1 || samples < 1 || long(Btraj) * samples > 0x7fffffffL || !(time_step > 0.) ||
        !std::isfinite(time_step) || substeps < 1 || max_steps < 1 || n_record < 0 || n_record > long(Btraj) * samples ||
        (n_record > 0 && write_steps < 1))
        return SCPP_E_ARG;
    if (int rc = readyToLaunch(c))
        return rc;
    if (!c->have_gains || (c->have_lim && c->lim_rows != 1 && c->lim_rows != c->B))
        return SCPP_E_STATE; // no gains, or limits for another number of trajectories
    if (Btraj != c->B)
        return SCPP_E_ARG; // `samples` starts per trajectory
    if (c->ffmode)
    {
        if (!c->have_ff)
            return SCPP_E_STATE; // no feedforward terms to fly
        if (c->hold)
            return SCPP_E_UNSUPPORTED; // the held loop's offset is another recursion
    }
    if (!allFinite(x_final, size_t(c->nx)))
        return SCPP_E_ARG;
    const int B = Btraj * samples; // flights
    DeviceGuard guard(c->device);
    if (int rc = growFlights(c, size_t(B)))
        return rc;
    if (write_steps < 1)
        write_steps = 1;
    const int rec_cap = n_record > 0 ? (max_steps + write_steps - 1) / write_steps : 0;
    if (n_record > 0 && (n_record > c->rec_alloc_inst || rec_cap > c->rec_alloc_rows))
    {
        // sized by n_record and the rows asked for, not by batch_max
        CHECK_HIP(hipStreamSynchronize(c->stream));
        void *old[] = {c->rx, c->ru, c->rt, c->rn};
        for (void *p : old)
            if (p)
                (void)hipFree(p);
        c->rx = c->ru = c->rt = nullptr;
        c->rn = nullptr;
        c->rec_alloc_inst = c->rec_alloc_rows = 0;
        const size_t rows = size_t(n_record) * rec_cap;
        if (devAlloc(&c->rx, rows * c->nx) | devAlloc(&c->ru, rows * c->nu) | devAlloc(&c->rt, rows) | devAlloc(&c->rn, size_t(n_record)))
            return SCPP_E_HIP;
        c->rec_alloc_inst = n_record;
        c->rec_alloc_rows = rec_cap;
    }
    CHECK_HIP(hipMemcpyAsync(c->xs, x_start, size_t(B) * c->nx * sizeof(double), hipMemcpyHostToDevice, c->stream));
    CHECK_HIP(hipMemcpyAsync(c->xf, x_final, size_t(c->nx) * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (c->have_noise)
    {
        for (int j = 0; j < c->nx; j++)
            c->noise_sd[j] = std::sqrt(c->noise_w[j] / time_step);
        CHECK_HIP(hipMemcpyAsync(c->nsd, c->noise_sd, size_t(c->nx) * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    if (!c->have_lim)
    {
        CHECK_HIP(hipMemsetAsync(c->onsat, 0, size_t(B) * sizeof(int), c->stream));
        CHECK_HIP(hipMemsetAsync(c->oclip, 0, size_t(B) * sizeof(double), c->stream));
    }
    const unsigned grid = unsigned((B + WAVE - 1) / WAVE);
    int rc = launchKernel(c, [&](auto pl) {
        using P = decltype(pl);
        // no limits: the SAT = false instantiation, which neither reads limits nor writes the saturation outputs
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(WAVE), 0, c->stream, B, samples, c->K, c->nU, c->uRows, c->tX, c->tU, c->tT,
                               (const double *)c->par, c->par_stride, (const double *)c->G, (const double *)c->xs, (const double *)c->xf, time_step,
                               substeps, c->stop_tol, max_steps, n_record, write_steps, rec_cap, c->ox, c->ou, c->os, c->oi, c->rx, c->ru, c->rt, c->rn,
                               (const double *)c->lim, c->lim_rows == 1 ? 0 : LIM_ROW, c->onsat, c->oclip,
                               (const double *)(c->ffmode ? c->ff : nullptr), (const double *)(c->have_noise ? c->nsd : nullptr), c->noise_seed,
                               c->noise_offset);
        };
        if (c->have_noise)
        {
            // the disturbed plant: the same six loops, NOISE = true
            if (c->ffmode)
            {
                if (c->have_lim)
                    go(lqr_track_kernel<P, true, false, true, true>);
                else
                    go(lqr_track_kernel<P, false, false, true, true>);
            }
            else if (c->hold)
            {
                if (c->have_lim)
                    go(lqr_track_kernel<P, true, true, false, true>);
                else
                    go(lqr_track_kernel<P, false, true, false, true>);
            }
            else if (c->have_lim)
                go(lqr_track_kernel<P, true, false, false, true>);
            else
                go(lqr_track_kernel<P, false, false, false, true>);
        }
        else if (c->ffmode)
        {
            if (c->have_lim)
                go(lqr_track_kernel<P, true, false, true>);
            else
                go(lqr_track_kernel<P, false, false, true>);
        }
        else if (c->hold)
        {
            if (c->have_lim)
                go(lqr_track_kernel<P, true, true>);
            else
                go(lqr_track_kernel<P, false, true>);
        }
        else if (c->have_lim)
            go(lqr_track_kernel<P, true>);
        else
            go(lqr_track_kernel<P, false>);
    });
    if (rc)
        return rc;
    CHECK_HIP(hipStreamSynchronize(c->stream)); // x_start / x_final are the caller's
    c->have_track = true;
    c->track_B = B;
    c->n_record = n_record;
    c->rec_cap = rec_cap;
    if (n_finite)
    {
        HostBuf<int> oi(size_t(B) * 2);
        if (!oi.p)
            return SCPP_E_HIP;
        CHECK_HIP(hipMemcpyAsync(oi.p, c->oi, oi.n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        CHECK_HIP(hipStreamSynchronize(c->stream));
        int n = 0;
        for (int b = 0; b < B; b++)
            n += (oi.p[size_t(b) * 2 + 1] != SCPP_LQR_NONFINITE);
        *n_finite = n;
    }
    return SCPP_OK;
}

int scpp_hip_lqr_track_download(scpp_hip_lqr_ctx *c, double *x, double *u, double *t, int *steps, int *status, double *err0, double *err1,
                                double *max_dev)
{
    if (!c)
        return SCPP_E_ARG;
    if (!c->have_track)
        return SCPP_E_STATE;
    DeviceGuard guard(c->device);
    const size_t B = size_t(c->track_B);
    HostBuf<double> osb(B * 4);
    HostBuf<int> oib(B * 2);
    if (!osb.p || !oib.p)
        return SCPP_E_HIP;
    double *os = osb.p;
    int *oi = oib.p;
    if (x)
        CHECK_HIP(hipMemcpyAsync(x, c->ox, B * c->nx * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (u)
        CHECK_HIP(hipMemcpyAsync(u, c->ou, B * c->nu * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    CHECK_HIP(hipMemcpyAsync(os, c->os, osb.n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    CHECK_HIP(hipMemcpyAsync(oi, c->oi, oib.n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    CHECK_HIP(hipStreamSynchronize(c->stream));
    for (size_t b = 0; b < B; b++)
    {
        if (t)
            t[b] = os[b * 4 + 0];
        if (err0)
            err0[b] = os[b * 4 + 1];
        if (err1)
            err1[b] = os[b * 4 + 2];
        if (max_dev)
            max_dev[b] = os[b * 4 + 3];
        if (steps)
            steps[b] = oi[b * 2 + 0];
        if (status)
            status[b] = oi[b * 2 + 1];
    }
    return SCPP_OK;
}

int scpp_hip_lqr_track_download_saturation(scpp_hip_lqr_ctx *c, int *n_sat, double *max_clip)
{
    if (!c)
        return SCPP_E_ARG;
    if (!c->have_track)
        return SCPP_E_STATE;
    DeviceGuard guard(c->device);
    const size_t F = size_t(c->track_B);
    if (n_sat)
        CHECK_HIP(hipMemcpyAsync(n_sat, c->onsat, F * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (max_clip)
        CHECK_HIP(hipMemcpyAsync(max_clip, c->oclip, F * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    CHECK_HIP(hipStreamSynchronize(c->stream));
    return SCPP_OK;
}

int scpp_hip_lqr_track_record_size(scpp_hip_lqr_ctx *c, int *n_record, int *rec_cap)
{
    if (!c)
        return SCPP_E_ARG;
    if (!c->have_track)
        return SCPP_E_STATE;
    if (n_record)
        *n_record = c->n_record;
    if (rec_cap)
        *rec_cap = c->rec_cap;
    return SCPP_OK;
}

int scpp_hip_lqr_track_record(scpp_hip_lqr_ctx *c, double *X, double *U, double *t, int *n)
{
    if (!c)
        return SCPP_E_ARG;
    if (!c->have_track || c->n_record < 1)
        return SCPP_E_STATE;
    DeviceGuard guard(c->device);
    // the kernel addresses the record with the row count of THIS call (rec_cap), whatever the allocation holds
    const size_t rows = size_t(c->n_record) * c->rec_cap;
    if (n)
        CHECK_HIP(hipMemcpyAsync(n, c->rn, size_t(c->n_record) * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (t)
        CHECK_HIP(hipMemcpyAsync(t, c->rt, rows * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (X)
        CHECK_HIP(hipMemcpyAsync(X, c->rx, rows * c->nx * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (U)
        CHECK_HIP(hipMemcpyAsync(U, c->ru, rows * c->nu * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    CHECK_HIP(hipStreamSynchronize(c->stream));
    return SCPP_OK;
}

int scpp_hip_lqr_synchronize(scpp_hip_lqr_ctx *c)
{
    if (!c)
        return SCPP_E_ARG;
    DeviceGuard guard(c->device);
    CHECK_HIP(hipStreamSynchronize(c->stream));
    return SCPP_OK;
}

} // extern "C"

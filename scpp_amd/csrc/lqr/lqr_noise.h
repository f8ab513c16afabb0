// Process noise of the tracking loop (scpp_hip_lqr_set_disturbance; the definition is in include/scpp_hip_lqr.h): a counter-based generator, so
// the standard normals z are a pure function of (seed, flight, plant step, state row) and no generator state exists anywhere.
//   philox4x32_10      the Philox4x32-10 block (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)
//   noiseUniform       52 bits of two output words -> a double strictly inside (0, 1), exactly
//   noiseNormalPair    one block -> two normals (Box-Muller)
// Plain C++ on purpose (64-bit products, no intrinsics): the device, the emulation and the host compile the same text.
#pragma once
#include <cmath>
#include <cstdint>

namespace scpp
{
namespace lqr
{

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u; // round multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u; // Weyl increments of the key

// out = Philox4x32-10(ctr, key); ten rounds, the key bumped between them (nine times)
__host__ __device__ inline void philox4x32_10(const uint32_t (&ctr)[4], const uint32_t (&key)[2], uint32_t (&out)[4])
{
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int round = 0; round < 10; round++)
    {
        const uint64_t p0 = uint64_t(PHILOX_M0) * c0, p1 = uint64_t(PHILOX_M1) * c2;
        const uint32_t n0 = uint32_t(p1 >> 32) ^ c1 ^ k0, n1 = uint32_t(p1), n2 = uint32_t(p0 >> 32) ^ c3 ^ k1, n3 = uint32_t(p0);
        c0 = n0;
        c1 = n1;
        c2 = n2;
        c3 = n3;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

// m = the 32 bits of hi and the upper 20 of lo (52 bits); u = (m + 0.5) 2^-52: m + 0.5 has 53 significant bits, so u is exact, and
// 2^-53 <= u <= 1 - 2^-53
__host__ __device__ inline double noiseUniform(uint32_t hi, uint32_t lo)
{
    const uint64_t m = (uint64_t(hi) << 20) | (lo >> 12);
    return (double(m) + 0.5) * 2.220446049250313e-16; // 2^-52
}

// z[2j], z[2j+1] of global flight g at plant step n: counter (n, j, g lo32, g hi32), key (seed lo32, seed hi32); |z| <= sqrt(106 ln 2) < 8.6
__host__ __device__ inline void noiseNormalPair(unsigned long long seed, unsigned long long g, uint32_t n, uint32_t j, double &z0, double &z1)
{
    const uint32_t ctr[4] = {n, j, uint32_t(g), uint32_t(g >> 32)}, key[2] = {uint32_t(seed), uint32_t(seed >> 32)};
    uint32_t c[4];
    philox4x32_10(ctr, key, c);
    const double u1 = noiseUniform(c[0], c[1]), u2 = noiseUniform(c[2], c[3]);
    const double rho = sqrt(-2. * log(u1));
    const double phi = 6.283185307179586 * u2;
    double sn, cs;
    sincos(phi, &sn, &cs); // one argument reduction for both
    z0 = rho * cs;
    z1 = rho * sn;
}

// z [flights][steps][nx] of the global flights flight0 .. and the plant steps step0 ..: one thread per (flight, step), the device function the
// tracking loop draws with (an odd nx drops the second normal of the last pair)
template <int NX>
__global__ void lqr_noise_kernel(unsigned long long seed, unsigned long long flight0, long flights, unsigned step0, int steps, double *__restrict__ z)
{
    constexpr int nx = NX;
    const long i = long(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= flights * steps)
        return;
    const unsigned long long g = flight0 + (unsigned long long)(i / steps);
    const uint32_t n = step0 + uint32_t(i % steps);
    for (int j = 0; 2 * j < nx; j++)
    {
        double z0, z1;
        noiseNormalPair(seed, g, n, uint32_t(j), z0, z1);
        z[i * nx + 2 * j] = z0;
        if (2 * j + 1 < nx)
            z[i * nx + 2 * j + 1] = z1;
    }
}

} // namespace lqr
} // namespace scpp

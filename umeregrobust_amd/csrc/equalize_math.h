// equalize_math.h -- the per-sample arithmetic of the sampling equalizer (equalize.hip, contract: equalize_api.h), written once: the
// integer mix behind the three random streams, the integer area weight and allocation, the f32 tangent basis and placement, and the fp64
// weight of the smoothing projection.  Every f32 line rounds once per operation (the build has -ffp-contract=off; parentheses give the
// order), every integer line is exact, so a host build of this text computes the device's bits.  Not part of the C ABI.
#pragma once
// UMEREG_EQUALIZE_HOST: the same text as plain C++, for a test harness that judges the routines on the CPU (tests/equalize_math_host.cpp);
// the device build does not define it.
#ifdef UMEREG_EQUALIZE_HOST
#include <cmath>
#include <cstdint>
#define UMEREG_EQ_FN inline
#else
#include "common.h"
#define UMEREG_EQ_FN __device__ inline
#endif

namespace umereg {

constexpr uint32_t kEqStreamStep = 0x9e3779b9u;   // 2^32 / golden ratio: separates the three streams of one seed

// "lowbias32" (C. Wellons, Hash Prospector, 2018: github.com/skeeto/hash-prospector): a bijection of the 32-bit words with an
// avalanche bias of 0.17
UMEREG_EQ_FN uint32_t eq_lowbias32(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// xi_c(j): the top 24 bits of the mix of (seed, j, c), c = 0 (allocation: j = 0 only), 1, 2 (placement).  Stateless: a function of its arguments.
UMEREG_EQ_FN uint32_t eq_xi(uint32_t seed, uint32_t j, uint32_t c)
{
    return eq_lowbias32(eq_lowbias32(seed + c * kEqStreamStep) + j) >> 8;
}

// the integer area weight of a surfel: q = (uint32)(r2 * s), s = (float)(65536 / r_max^2); r2 <= r_max^2, so q <= 65537
UMEREG_EQ_FN uint32_t eq_area_weight(float r2, float s)
{
    return (uint32_t)(r2 * s);
}

// systematic allocation: the position of sample j of M on the axis [0, Qt) of the summed weights, u_j = (j Qt + r) / M with the one
// offset r = (xi0 Qt) >> 24 < Qt that all samples of a call share (xi0 = xi_0(0)).  u_j is the floor of the real comb (j + r / Qt) Qt / M,
// and an integer interval holds floor(x) exactly when it holds x: a point that owns q of the axis gets floor or ceil of its share
// M q / Qt, so |count - share| < 1.  j < M <= 2^22 and Qt <= 2^22 * 65537 keep j * Qt + r below 2^61, xi0 < 2^24 keeps xi0 * Qt below
// 2^63.  u < Qt always; Qt < M (several samples on one position) is legal.
UMEREG_EQ_FN uint64_t eq_alloc(uint64_t j, uint64_t Qt, uint64_t M, uint32_t xi0)
{
    const uint64_t r = ((uint64_t)xi0 * Qt) >> 24;
    return (j * Qt + r) / M;
}

// the branch-free orthonormal basis of a unit normal (Duff, Burgess, Christensen, Hery, Kensler, Liani, Villemin: "Building an
// Orthonormal Basis, Revisited", JCGT 6(1), 2017), in f32
UMEREG_EQ_FN void eq_basis(const float (&n)[3], float (&t1)[3], float (&t2)[3])
{
    const float sign = copysignf(1.0f, n[2]);
    const float a = -1.0f / (sign + n[2]);
    const float b = (n[0] * n[1]) * a;
    t1[0] = 1.0f + ((sign * n[0]) * n[0]) * a;
    t1[1] = sign * b;
    t1[2] = -sign * n[0];
    t2[0] = b;
    t2[1] = sign + (n[1] * n[1]) * a;
    t2[2] = -n[1];
}

// xi (24 bits) -> [-1, 1): (xi - 2^23) * 2^-23, exact in f32
UMEREG_EQ_FN float eq_unit(uint32_t xi)
{
    return (float)((int32_t)xi - 8388608) * 0x1p-23f;
}

// sample position on the square patch of a surfel: half side h = sqrtf(r2) * c with c = (float)(0.5 sqrt(pi / K)), so that the patch area
// is the point's share pi r_k^2 / K of its neighbourhood disc; x = p + h * (a * t1 + b * t2)
UMEREG_EQ_FN void eq_place(const float (&p)[3], const float (&n)[3], float r2, float c, uint32_t xi1, uint32_t xi2, float (&x)[3])
{
    float t1[3], t2[3];
    eq_basis(n, t1, t2);
    const float a = eq_unit(xi1), b = eq_unit(xi2);
    const float h = sqrtf(r2) * c;
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = p[k] + h * ((a * t1[k]) + (b * t2[k]));
}

// the library's predicate distance: f32, ((dx*dx) + (dy*dy)) + (dz*dz)
UMEREG_EQ_FN float eq_d2(float dx, float dy, float dz)
{
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}

// weight of a neighbour at squared distance d2 < rho2 in the projection: (1 - d2 / rho2)^2 in fp64 (a polynomial: no exp)
UMEREG_EQ_FN double eq_weight(float d2, float rho2)
{
    const double t = 1.0 - (double)d2 / (double)rho2;
    return t * t;
}

}  // namespace umereg

// Counter-based Gaussian noise for the stochastic samplers (DPM-Solver++ 2M SDE, Euler-ancestral):
// Philox4x32-10 and a Box-Muller transform.  Plain functions over words, compiled as they stand by
// latent_step_noise_kernel (misc.hip, one lane per latent pixel) and by a host program
// (tests/native/philox_normal_host.cpp).  models/schedulers.py holds the numpy model
// (philox4x32, philox_normal).
//
// NOISE CONTRACT.  Latents are NHWC with 4 channels.  For image b with 64-bit seed S_b, eval index
// s (the device step counter) and pixel p of that image (p = j / 4 for element j of the image):
//     key     = (low 32 bits of S_b, high 32 bits of S_b)
//     counter = (p, s, 0, 0)
//     w0..w3  = Philox4x32-10(counter, key)
//     u_i     = ((w_i >> 8) + 0.5) * 2^-24                       (in (0, 1), never 0 or 1)
//     channels 0, 1:  r = sqrt(-2 ln u_0),  z_0 = r cos(2 pi u_1),  z_1 = r sin(2 pi u_1)
//     channels 2, 3:  the same from u_2, u_3
// so the noise of an image depends on its seed, the eval and the pixel alone: not on the batch the
// image sits in, nor on its position there.  |z| <= sqrt(2 * 25 * ln 2) < 5.9.
//
// fp32 evaluation (agrees with the float64 model within 1e-5 * max(1, |z|)):
//  * (k + 0.5) is not a float once k >= 2^23, and ln u loses everything near u = 1, so for the
//    upper half ln u = log1p(-(2^24 - k - 0.5) * 2^-24), whose argument is exact;
//  * the angle is reduced exactly in integers: 2 pi u = (2k + 1) * 2^-25 turns = quadrant
//    (2k + 1) >> 23 plus a fraction f * 2^-23 of a quarter turn with f < 2^23 exact in a float;
//    sin and cos are taken on [0, pi / 2) and rotated by the quadrant.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define PHILOX_FN __host__ __device__ inline
#else
#define PHILOX_FN inline
#endif

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;   // multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;   // Weyl key increments

// Philox4x32-10: c[4] (counter) -> c[4] (output words), key (k0, k1)
PHILOX_FN void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)PHILOX_M0 * c[0], p1 = (uint64_t)PHILOX_M1 * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1;
    c[3] = (uint32_t)p0;
    c[0] = n0;
    c[2] = n2;
    k0 += PHILOX_W0;
    k1 += PHILOX_W1;
  }
}

// one Box-Muller pair from two words
PHILOX_FN void philox_box_muller(uint32_t w0, uint32_t w1, float* z0, float* z1) {
  const uint32_t k = w0 >> 8;
  const float ln_u = k < (1u << 23) ? logf(((float)k + 0.5f) * 0x1p-24f)
                                    : log1pf(-((float)((1u << 24) - k) - 0.5f) * 0x1p-24f);
  const float r = sqrtf(-2.f * ln_u);
  const uint32_t t = 2u * (w1 >> 8) + 1u;                       // angle in units of 2^-25 turn
  const float phi = (float)(t & ((1u << 23) - 1u)) * (1.57079632679489662f * 0x1p-23f);
  const float s = sinf(phi), c = cosf(phi);
  const uint32_t q = t >> 23;                                   // quadrant 0..3
  const float cq = (q & 1u) ? -s : c, sq = (q & 1u) ? c : s;    // rotate by q quarter turns
  *z0 = r * ((q & 2u) ? -cq : cq);
  *z1 = r * ((q & 2u) ? -sq : sq);
}

// the four normals of one latent pixel (NOISE CONTRACT above); w: the four Philox words
PHILOX_FN void philox_normal4(uint32_t seed_lo, uint32_t seed_hi, uint32_t pixel, uint32_t step, uint32_t w[4],
                              float z[4]) {
  w[0] = pixel; w[1] = step; w[2] = 0u; w[3] = 0u;
  philox4x32_10(w, seed_lo, seed_hi);
  philox_box_muller(w[0], w[1], &z[0], &z[1]);
  philox_box_muller(w[2], w[3], &z[2], &z[3]);
}

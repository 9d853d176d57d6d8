// Counter-based Gumbel noise for the LM decode sampler: Philox4x32-10 (philox_normal.h) and
// g = -ln(-ln u).  Plain functions over words, compiled as they stand by lm_sample_seeded_kernel
// and lm_gumbel_kernel (lm_sample.hip) and by a host program
// (tests/native/philox_gumbel_host.cpp).  models/schedulers.py holds the numpy model
// (philox_gumbel).
//
// GUMBEL CONTRACT.  For a sequence with 64-bit seed S, decode step s (the sequence's own step
// counter, its low 32 bits) and vocabulary id i:
//     key     = (low 32 bits of S, high 32 bits of S)            (schedulers.seed_key)
//     counter = (i >> 2, s, 0, 0)
//     w       = Philox4x32-10(counter, key)[i & 3]
//     u       = ((w >> 8) + 0.5) * 2^-24                          (in (0, 1), never 0 or 1)
//     g       = -ln(-ln u)                                        (in [-2.853, 17.329])
// so the noise of a token depends on the seed, the step and the id alone: not on the batch the
// sequence sits in, its row there, the sampler's k or the other logits.
//
// fp32 evaluation (agrees with the float64 model within 2e-6 * max(1, |g|)): ln u as
// philox_box_muller takes it, logf below k = 2^23 where (k + 0.5) * 2^-24 is exact, log1pf of the
// exact complement above (ln u loses everything near u = 1 otherwise); then -logf(-ln u).  A
// relative error e of ln u is an absolute error e of g, so a few ulp of logf / log1pf and a few
// of the outer logf stay near 1e-7 * max(1, |g|).
#pragma once
#include "philox_normal.h"

// ln u of a word's top 24 bits, u = ((w >> 8) + 0.5) * 2^-24
PHILOX_FN float philox_ln_u(uint32_t w) {
  const uint32_t k = w >> 8;
  return k < (1u << 23) ? logf(((float)k + 0.5f) * 0x1p-24f)
                        : log1pf(-((float)((1u << 24) - k) - 0.5f) * 0x1p-24f);
}

// the Gumbel variate of one word
PHILOX_FN float philox_gumbel_word(uint32_t w) { return -logf(-philox_ln_u(w)); }

// the word of vocabulary id `id` at decode step `step` (GUMBEL CONTRACT above)
PHILOX_FN uint32_t philox_gumbel_bits(uint32_t seed_lo, uint32_t seed_hi, uint32_t id, uint32_t step) {
  uint32_t c[4] = {id >> 2, step, 0u, 0u};
  philox4x32_10(c, seed_lo, seed_hi);
  const uint32_t lane = id & 3u;                      // selects without indexing c[] at run time
  return lane == 0u ? c[0] : lane == 1u ? c[1] : lane == 2u ? c[2] : c[3];
}

PHILOX_FN float philox_gumbel(uint32_t seed_lo, uint32_t seed_hi, uint32_t id, uint32_t step) {
  return philox_gumbel_word(philox_gumbel_bits(seed_lo, seed_hi, id, step));
}

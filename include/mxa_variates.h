/* mxa_variates.h - the probe of the run kernel's variate tables: a part of the C-ABI of include/mxa.h
 * (which includes this file).  Same conventions: 0 or a negative MXA_E* code. */
#ifndef MXA_VARIATES_H
#define MXA_VARIATES_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* A variate table is a positional memo over up to 64 doubles of one MT19937 stream: the
 * exponential's log and the polar method's two normals of every double pair, computed lane-parallel
 * when a draw misses and read back by the draws that follow (DESIGN.md section 3 "Variate tables").
 * The probe runs `n` draws of `script` (one byte each: 0 standard exponential, 1 standard normal,
 * 2 one 32-bit word, 3 randint(0, 100)) on a stream seeded as numpy.random.RandomState(seed), on one
 * wave, twice: through a table, with the device functions the engine's value agents draw with, and
 * through the serial draws alone.
 *   out   HOST [2][n] float64: the values of the table pass, then of the serial pass
 *   state HOST [2][n][3] uint64: the stream's (position, gauss flag, cached gauss bits) after every draw
 * `lookahead` (2 .. 256) caps the words a fill may span from the draw's position (the engine's is
 * MXA_AGENT_LA = 256, more than the 128 words of a full table).  The two passes must agree bit for
 * bit in both arrays.  MXA_EINVAL before any HIP call: null pointer, n < 1, lookahead outside 2 .. 256
 * or a script byte above 3.  Synchronous. */
int mxa_variate_probe(int32_t device, uint32_t seed, const uint8_t* script, int32_t n, int32_t lookahead, double* out,
                      uint64_t* state);

#ifdef __cplusplus
}
#endif
#endif

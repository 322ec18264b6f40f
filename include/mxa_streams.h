/* mxa_streams.h - the probe of the build kernel's head streams: a part of the C-ABI of include/mxa.h
 * (which includes this file).  Same conventions: 0 or a negative MXA_E* code. */
#ifndef MXA_STREAMS_H
#define MXA_STREAMS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* The build kernel materialises of an agent's own MT19937 stream only what the run can read
 * (DESIGN.md section 4 "RNG streams"): everything for a class that draws at every wake, the first
 * words of block 1 (the head) for a NoiseAgent or a MomentumAgent, whose one draw is a
 * randint, and nothing for a class that never draws.  A draw that leaves a head sets the stream's
 * overrun flag (bit 1 of the flag word), which stops the env with error 9 at the event's end.
 * The probe seeds one stream as numpy.random.RandomState(seed) through the head path with a head
 * of `head_words` (2 .. 64; the engine's is 64) outputs, on one wave, and makes `n` randint(0, 100)
 * draws with the device functions the engine's wake_frequency uses.
 *   out_values HOST [n] float64: the draws
 *   out_state  HOST [n][2] uint64: the stream's (position, flag word) after every draw
 * A draw whose words all lie inside the head equals numpy's and leaves bit 1 clear; the first draw
 * that consumes word `head_words` sets it, and it stays set.  MXA_EINVAL before any HIP call: null
 * pointer, n < 1 or head_words outside 2 .. 64.  Synchronous. */
int mxa_stream_head_probe(int32_t device, uint32_t seed, int32_t head_words, int32_t n, double* out_values,
                          uint64_t* out_state);

#ifdef __cplusplus
}
#endif
#endif

// wavenet_stream.h -- the host rules the two precisions of the streaming WaveNet layer share (csrc/wavenet_stream.hip:
// fp32, where they are defined; csrc/wavenet_stream_bf16.hip: bf16 operands): which layers a stream launch covers and
// which pointers it takes.  Both precisions admit the same layers, delays and buffers, and refuse the rest with the same
// words in pwg_last_error.  Shared between two translation units but not exported from the library.
#pragma once
#include "common.h"

#include <stdint.h>

namespace pwg {

// delayed: the look-ahead form, whose descriptor is the non-causal layer's own
__attribute__((visibility("hidden"))) int wavenet_stream_geometry(const pwg_wavenet_desc* d, bool delayed = false);

// What the delayed form adds to it: the aux window starts c_delay columns early, inside a line of at least as many
__attribute__((visibility("hidden"))) int wavenet_delayed_geometry(const pwg_wavenet_desc* d, int32_t c_delay);

// The pointer rules of both forms: what must be there, what must not alias, alignment (the weight image: 16 B)
__attribute__((visibility("hidden"))) int wavenet_stream_pointers(const char* name, const float* x, const float* c,
                                                                  const float* hist_in, const float* hist_out,
                                                                  const void* packed, const float* x_out,
                                                                  const float* skips_out);

// ... and of the delayed form's lines
__attribute__((visibility("hidden"))) int wavenet_delayed_pointers(const char* name, const pwg_wavenet_desc* d,
                                                                   const float* c_line, int32_t c_cols, int32_t c_delay,
                                                                   const float* skips, const float* skip_line_in,
                                                                   const float* skip_line_out, const float* skips_out);

// ... and what the slotted form asks beyond them: the table, its rate and delay, and every state input the delayed form
// may leave NULL (the start of a stream is an item's, in the table; a launch-wide NULL has no meaning)
__attribute__((visibility("hidden"))) int wavenet_slots_pointers(const char* name, const pwg_wavenet_desc* d,
                                                                 int32_t c_delay, const float* c_line, const float* skips,
                                                                 const float* skip_line_in, const float* hist_in,
                                                                 const int32_t* slots, int32_t rate, int32_t delay);

}  // namespace pwg

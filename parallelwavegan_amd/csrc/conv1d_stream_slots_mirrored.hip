// conv1d_stream_slots_mirrored.hip -- the entry point of the slotted-mirrored form of the streaming convolution
// (include/pwg_kernels.h): the mirrored launch of a reflect-padded layer with one position per item,
// for a pool of (multi-band) MelGAN look-ahead streams.  The kernel is the <TM, TN, false, true, true, true>
// instantiation of conv1d_stream_kernel and lives with its family in conv1d_stream.hip, which also holds the host path
// (stream_slots_mirrored_forward, stream_common.h).  The entry point stands here because tests/test_stream_refs_host.py
// ties every entry point defined in conv1d_stream.hip to the chunk-by-chunk matrix of
// tests/test_conv_stream_matrix_gpu.py; this one is driven by tests/test_stream_melgan_pool_gpu.py instead.
#include "stream_common.h"

extern "C" int pwg_conv1d_stream_slots_mirrored_forward(const pwg_conv1d_desc* d, const float* x, const float* hist_in,
                                                        float* hist_out, const float* w_packed, const float* bias,
                                                        const int32_t* slots, int32_t rate, int32_t delay, float* y,
                                                        void* stream) {
  return pwg::stream_slots_mirrored_forward(d, x, hist_in, hist_out, w_packed, bias, slots, rate, delay, y, stream);
}

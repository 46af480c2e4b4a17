// jpeg_stream_core.h — where the samples of dvc_jpeg_encode_stream lie
// (DESIGN.md "Motion-JPEG stream", "Stream output"), as plain C++ that compiles
// for the device (k_jpeg_stream_offsets and k_jpeg_stream_gather in
// jpeg_kernels.hip) and for the host (tools/jpeg_stream_host_check.cc runs the
// same text under the host sanitizers): a sample's bytes from its segments'
// lengths, the exclusive prefix over a launch group with the carry of the
// groups before it, the test whether a sample lies inside the caller's buffer,
// and a segment's place inside its sample. All of it in 64 bits: a call's
// total may pass 2^32.
#pragma once
#include <stdint.h>

#ifndef DVC_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DVC_HD __host__ __device__ __forceinline__
#else
#define DVC_HD inline
#endif
#endif

namespace dvc {

// The bytes segments first, first + step, .. below `end` take in a sample: each
// with the 2-byte marker behind it (RSTm, or EOI after the last). A lane's
// part of the sum (first = lane, step = lanes), or all of it (0, 1).
DVC_HD uint64_t stream_seg_sum(const uint32_t* seglen, int end, int first, int step)
{
    uint64_t sum = 0;
    for (int i = first; i < end; i += step) sum += (uint64_t)seglen[i] + 2u;
    return sum;
}

// A complete sample: the handle's header, the table group's DHT + SOS prefix
// (0 with fixed tables), the segments and their markers.
DVC_HD uint64_t stream_frame_need(uint32_t header_len, uint32_t prefix_len, uint64_t seg_sum)
{
    return (uint64_t)header_len + prefix_len + seg_sum;
}

// A sample is written iff it lies wholly inside the caller's `cap` bytes.
DVC_HD bool stream_fits(uint64_t end, uint64_t cap) { return end <= cap; }

// The exclusive prefix of a launch group's m samples behind `carry`, the end
// of the groups before it: offsets[t] is where sample t starts, offsets[m]
// where the group ends, which is the next group's carry and is returned.
// *overflow is set when a sample does not fit `cap`; it is never cleared here.
DVC_HD uint64_t stream_group_offsets(const uint64_t* need, int m, uint64_t carry, uint64_t cap, uint64_t* offsets,
                                     uint32_t* overflow)
{
    uint64_t at = carry;
    for (int t = 0; t < m; ++t) {
        offsets[t] = at;
        at += need[t];
        if (!stream_fits(at, cap)) *overflow = 1u;
    }
    offsets[m] = at;
    return at;
}

// Where segment s of a sample begins, counted from the sample's start:
// `before` = stream_seg_sum over the segments below s.
DVC_HD uint64_t stream_seg_start(uint32_t header_len, uint32_t prefix_len, uint64_t before)
{
    return (uint64_t)header_len + prefix_len + before;
}

}  // namespace dvc

/* dvc_jpeg_stream.h - the stream output of the Motion-JPEG encoder
 * (include/dvc.h, dvc_jpeg_*): complete samples, back to back, ready to be
 * written to a file as they are. An addition to the C-ABI of dvc.h, version 10,
 * exported by the same library; it is a header of its own because dvc.h's set of
 * prototypes is pinned. DESIGN.md "Motion-JPEG stream", "Stream output" is the
 * normative text. */
#ifndef DVC_JPEG_STREAM_H
#define DVC_JPEG_STREAM_H

#include "dvc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Encode n frames (pointer, pitch and stride rules of dvc_jpeg_encode) into
 * out[0 .. cap): sample t occupies out[offsets[t] .. offsets[t+1]) and is
 * exactly the bytes of dvc_jpeg_header(h) followed by the bytes
 * dvc_jpeg_encode writes for frame t - with DVC_FLAG_JPEG_OPT_HUFFMAN the short
 * header, the table group's DHT and SOS segments, the data and EOI; a table
 * group is a run of max_batch frames of one call, as there. offsets has n + 1
 * entries, offsets[0] = 0, offsets[n] is the total; nothing lies between two
 * samples, so a sample starts at any byte alignment.
 * A sample that does not lie wholly inside cap is not written, no byte at or
 * past out + cap ever is, offsets still holds the needed values of all n frames
 * and the call returns DVC_E_NOMEM - on a DVC_FLAG_DEVICE_PTRS handle the next
 * dvc_jpeg_sync does (dvc_jpeg_encode's rule).
 * On a DVC_FLAG_DEVICE_PTRS handle frames, out and offsets (8-byte aligned) are
 * device pointers and the call is asynchronous on the handle's stream; on a
 * host handle they are host pointers, the call stages on the device, brings
 * offsets and then offsets[n] bytes down and returns when they are there.
 * DVC_E_STATE on a handle without a device; DVC_E_INVALID for a NULL argument,
 * n < 0, a pitch or frame stride dvc_jpeg_encode refuses. */
int dvc_jpeg_encode_stream(dvc_jpeg* h, const uint8_t* frames, size_t pitch, size_t frame_stride, int n,
                           uint8_t* out, size_t cap, uint64_t* offsets);

#ifdef __cplusplus
}
#endif

#endif /* DVC_JPEG_STREAM_H */

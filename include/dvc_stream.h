/* dvc_stream.h - a HIP stream for callers that have no HIP binding of their own
 * (the Python drivers): created here, handed to the create calls of dvc.h as
 * hip_stream so that several handles join it, and destroyed when the run ends, so
 * that a run leaves no stream behind. An addition to the C-ABI of dvc.h, version
 * 10, exported by the same library; a header of its own because dvc.h's set of
 * prototypes is pinned. */
#ifndef DVC_STREAM_H
#define DVC_STREAM_H

#include "dvc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A non-blocking stream on `device`. DVC_E_INVALID for a NULL argument, DVC_E_HIP
 * when the runtime refuses. */
int dvc_stream_create(int device, void** stream);
/* Wait for the stream's work, then destroy it; every handle that joined it must
 * have been destroyed before. NULL is ignored. */
int dvc_stream_destroy(int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DVC_STREAM_H */

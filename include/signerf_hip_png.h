/*
 * signerf_hip_png.h -- companion header of signerf_hip.h: a device uint8 image to the bytes of its .png file, encoded on the GPU.  The
 * generator's images are cast to uint8 on the device (sn_tensor_to_uint8); with this call the finished FILE crosses PCIe instead of the
 * pixels, and no host thread deflates.  Exported from the same libsignerf_hip.so and following the conventions of signerf_hip.h (int
 * status, sn_last_error, caller-owned device memory, work enqueued on the caller's stream, no hidden sync).
 *
 * The file: 8-bit greyscale (c = 1) or RGB (c = 3), one IDAT chunk holding one zlib stream (header 78 01) over the filtered scanlines --
 * row 0 with filter 0, every other row with filter 2 ("Up").  The stream is cut into segments of sn_png_segment_bytes() bytes; a segment
 * is deflated on its own into one block (stored, fixed or dynamic Huffman, whichever occupies the fewest bytes) by a matcher that tries a
 * fixed list of distances, so a file's bytes are a pure function of (pixels, shape): DESIGN.md §4 "PNG encoding".  Any PNG reader reads it.
 *
 * Versioning: SN_PNG_ABI_VERSION / sn_png_abi_version() version THIS header's signatures.
 */
#ifndef SIGNERF_HIP_PNG_H
#define SIGNERF_HIP_PNG_H

#include "signerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SN_PNG_ABI_VERSION 1
int sn_png_abi_version(void);

/* Bytes of the filtered stream one deflate block covers. */
size_t sn_png_segment_bytes(void);

/* Exact upper bound of the file of an [h, w, c] image (every segment stored), and the workspace sn_png_encode needs for it.
 * Both are 0 for a shape sn_png_encode refuses: c not 1 or 3, h or w outside 1..8192. */
size_t sn_png_max_file_bytes(int32_t h, int32_t w, int32_t c);
size_t sn_png_workspace_bytes(int32_t h, int32_t w, int32_t c);

/* Encodes image (DEVICE uint8 [h, w, c], contiguous) into file (DEVICE, file_capacity >= sn_png_max_file_bytes bytes) and writes the
 * file's byte count to file_bytes (DEVICE uint64).  workspace: DEVICE, 16-byte aligned, workspace_bytes >= sn_png_workspace_bytes;
 * its content before the call does not matter and nothing of it outlives the call.  Three kernels on `stream`; nothing is synchronised.
 * SN_ERR_INVALID with a text in sn_last_error(NULL), before any launch: a NULL pointer, c not in {1, 3}, h or w outside 1..8192, a
 * workspace (or its alignment) or a capacity below what the size queries return. */
int sn_png_encode(const uint8_t* image, int32_t h, int32_t w, int32_t c, void* workspace, size_t workspace_bytes, uint8_t* file,
                  size_t file_capacity, uint64_t* file_bytes, SnStream stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGNERF_HIP_PNG_H */

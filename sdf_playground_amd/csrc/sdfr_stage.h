// sdfr_stage.h -- how one device buffer is cut into the pieces a call needs: the stand-ins of a caller's host arrays (queries, mesh
// extraction, atlas) or the parts of a workspace.  Plain host arithmetic, no HIP call, so that it can be checked on a machine without a GPU
// (tests/test_stage_cpu.py); the helper that reserves the buffer and copies the answers back is Carving (sdfr_handle.h).
#pragma once
#include <stddef.h>

namespace sdfr {

enum { SDFR_STAGE_ALIGN = 256, SDFR_STAGE_MAX_PIECES = 8 }; // the atlas names seven: three inputs, four answers

// pieces of bytes[0 .. n) one after the other, each starting on a multiple of SDFR_STAGE_ALIGN (a piece of no bytes takes no room):
// offsets[k] = where piece k starts; returns the bytes of the whole
inline size_t stage_offsets(const size_t *bytes, int n, size_t *offsets)
{
	size_t at = 0;
	for (int k = 0; k < n; ++k)
	{
		offsets[k] = at;
		at += (bytes[k] + (SDFR_STAGE_ALIGN - 1)) & ~(size_t)(SDFR_STAGE_ALIGN - 1);
	}
	return at;
}

} // namespace sdfr

"""Host (numpy) statements of the multi-GPU strip layout (include/sdfr.h, "Multi-GPU"): what the CPU tests of the multi-rank path hold
sdfr_render_strips / sdfr_assemble_strips and the packed wire formats against."""
import numpy as np

from ._abi import STRIP_ROWS


def _shared_index(strip, split):
    """Index of a frame strip among the shared strips, or None if it is private (split = (m, M))."""
    m, M = split
    if m == 0:
        return strip
    j = strip % M
    return None if j < m else (strip // M) * (M - m) + (j - m)


def assemble_strips_host(width, height, world, gathered, split=(0, 1), image=None):
    """Host (numpy) statement of the strip layout: gathered[world, strip_buffer_pixels, C] ->
    image[height, width, C] (private strips of `split` are left as they are in `image`).  Used by
    the CPU tests of the multi-rank path; the GPU path is sdfr_assemble_strips."""
    gathered = np.asarray(gathered)
    C = gathered.shape[-1]
    per_rank_rows = strip_buffer_pixels_host(width, height, world, split) // width
    g = gathered.reshape(world, per_rank_rows, width, C)
    img = np.zeros((height, width, C), gathered.dtype) if image is None else image
    for py in range(height):
        t = _shared_index(py // STRIP_ROWS, split)
        if t is not None:
            img[py] = g[t % world, (t // world) * STRIP_ROWS + py % STRIP_ROWS]
    return img


def pack_strip_host(compact_rgba):
    """Host statement of SDFR_STRIP_RGB32F_A8: [n, 4] float32 (alpha 0 or 1) -> uint8 buffer of
    (13 n + 3) // 4 * 4 bytes: n rgb float triples, then n flag bytes."""
    c = np.ascontiguousarray(compact_rgba, np.float32).reshape(-1, 4)
    n = c.shape[0]
    out = np.zeros(((13 * n + 3) // 4 * 4,), np.uint8)
    out[:12 * n] = np.ascontiguousarray(c[:, :3]).view(np.uint8).reshape(-1)
    out[12 * n:13 * n] = (c[:, 3] != 0).astype(np.uint8)
    return out


def unpack_strip_host(packed, n):
    """Inverse of pack_strip_host: -> [n, 4] float32."""
    packed = np.asarray(packed, np.uint8)
    c = np.zeros((n, 4), np.float32)
    c[:, :3] = packed[:12 * n].view(np.float32).reshape(n, 3)
    c[:, 3] = packed[12 * n:13 * n].astype(np.float32)
    return c


def pack_strip16_host(compact_rgba):
    """Host statement of SDFR_STRIP_RGB16F_A8: [n, 4] float32 (alpha 0 or 1) -> uint8 buffer of
    (7 n + 3) // 4 * 4 bytes: n rgb half triples (round to nearest even), then n flag bytes."""
    c = np.ascontiguousarray(compact_rgba, np.float32).reshape(-1, 4)
    n = c.shape[0]
    out = np.zeros(((7 * n + 3) // 4 * 4,), np.uint8)
    with np.errstate(over="ignore"):
        out[:6 * n] = np.ascontiguousarray(c[:, :3].astype(np.float16)).view(np.uint8).reshape(-1)
    out[6 * n:7 * n] = (c[:, 3] != 0).astype(np.uint8)
    return out


def unpack_strip16_host(packed, n):
    """Inverse of pack_strip16_host: -> [n, 4] float16 (the RGBA16F pixels)."""
    packed = np.asarray(packed, np.uint8)
    c = np.zeros((n, 4), np.float16)
    c[:, :3] = packed[:6 * n].view(np.float16).reshape(n, 3)
    c[:, 3] = packed[6 * n:7 * n].astype(np.float16)
    return c


def strip_buffer_pixels_host(width, height, world, split=(0, 1)):
    strips = (height + STRIP_ROWS - 1) // STRIP_ROWS
    shared = sum(1 for s in range(strips) if _shared_index(s, split) is not None)
    return ((shared + world - 1) // world) * STRIP_ROWS * width


def private_rows_host(height, split):
    """Global rows of the private strips (rendered by the root straight into the image)."""
    return [r for r in range(height) if _shared_index(r // STRIP_ROWS, split) is None]


def strip_rows_of_rank(height, rank, world, split=(0, 1)):
    """Global rows of the shared strips owned by `rank`, in the order they appear in its compact buffer."""
    rows = []
    strips = (height + STRIP_ROWS - 1) // STRIP_ROWS
    for s in range(strips):
        t = _shared_index(s, split)
        if t is None or t % world != rank:
            continue
        for k in range(STRIP_ROWS):
            if s * STRIP_ROWS + k < height:
                rows.append(s * STRIP_ROWS + k)
    return rows

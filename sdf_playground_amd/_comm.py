"""Comm: the library's RCCL communicator (sdfr_comm_*, include/sdfr.h "multi-GPU in the library itself")."""
import ctypes
import sys

from ._abi import COMM_ID_BYTES, SDFR_OK, SdfrError, load_library


class Comm:
    """One RCCL communicator per process and GPU (sdfr_comm_*).  Rank 0 makes the id with
    Comm.unique_id() and hands it to the other ranks by any means (bench.py: torch.distributed
    broadcast); creation is collective."""

    @staticmethod
    def _one_rccl_per_process():
        """PyTorch ships a librccl of its own (torch/lib/librccl.so) and loads it by PATH, whatever the process holds
        already.  libsdfr.so opens a copy the process maps before any other (sdfr_comm.cpp), so the process runs one RCCL
        if torch's is there FIRST; a process that made a communicator and imported torch afterwards would run two.
        load_library() imports torch already (one HIP runtime); this keeps the property where someone loads the
        library by other means."""
        if "torch" not in sys.modules:
            try:
                import torch  # noqa: F401
            except ImportError:
                pass

    @staticmethod
    def _check(rc, comm=None):
        """comm: the communicator whose error text is wanted; None: the text of the call that has none (yet, or any more)"""
        if rc != SDFR_OK:
            raise SdfrError(rc, load_library().sdfr_comm_last_error(comm).decode())

    @staticmethod
    def library_info():
        """(path of the librccl serving libsdfr.so, ncclGetVersion code, distinct librccl files mapped by the process)"""
        Comm._one_rccl_per_process()
        path = ctypes.create_string_buffer(1024)
        version, copies = ctypes.c_int(0), ctypes.c_int(0)
        Comm._check(load_library().sdfr_comm_library_info(path, len(path), ctypes.byref(version), ctypes.byref(copies)))
        return path.value.decode(), version.value, copies.value

    @staticmethod
    def unique_id():
        Comm._one_rccl_per_process()
        buf = ctypes.create_string_buffer(COMM_ID_BYTES)
        Comm._check(load_library().sdfr_comm_unique_id(buf))
        return bytes(buf.raw)

    def __init__(self, uid, rank, world, device=0):
        Comm._one_rccl_per_process()
        self._L = load_library()
        self._c = ctypes.c_void_p()
        assert len(uid) == COMM_ID_BYTES
        self._check(self._L.sdfr_comm_create(ctypes.c_char_p(uid), int(rank), int(world), int(device), ctypes.byref(self._c)))
        self.rank, self.world, self.device = int(rank), int(world), int(device)

    def selftest(self, nbytes=1 << 20, stream_handle=None):
        """Ring exchange of nbytes over the communicator, compared at the destination (blocking)."""
        self._check(self._L.sdfr_comm_selftest(self._c, int(nbytes), ctypes.c_void_p(stream_handle)), self._c)
        return True

    def close(self):
        """sdfr_comm_close: drains the streams the communicator's transfers ran on, then ncclCommFinalize + ncclCommDestroy,
        bounded in time (SDFR_COMM_CLOSE_TIMEOUT_S, default 30 s): a teardown that does not finish raises SdfrError with the
        call it was stuck in instead of holding the process.  Collective in effect -- every rank closes.  Not called
        implicitly (a communicator still open when the process ends is reclaimed with it)."""
        if self._c:
            c, self._c = self._c, ctypes.c_void_p()
            self._check(self._L.sdfr_comm_close(c))

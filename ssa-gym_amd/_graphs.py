"""Capturing a hipGraph so that a capture that fails does not end the process: for parallel.GraphedShardedSteps and envs/_policy.py."""
import ctypes
import gc

import torch


def _never_destroy(graph):
    """a torch.cuda.CUDAGraph whose capture FAILED must not be finalised: capture_end() threw before the graph let go of the RNG generator
    state it registered with, and in this torch build (2.10 + ROCm 7) its destructor then fails a TORCH_CHECK ("The graph should be registered
    to the state") -- an exception out of a C++ destructor: the process aborts, whenever the object happens to be freed (at the return of the
    capturing function, or later by the garbage collector).  One leaked reference keeps the few hundred bytes alive for the life of the
    process (tests/test_env_gpu.py::test_run_policy_replayed_from_a_graph_equals_the_eager_loop)."""
    ctypes.pythonapi.Py_IncRef(ctypes.py_object(graph))


def _end_stray_capture(streams):
    """after a failed capture: none of `streams` may be left in capture mode (hipStreamIsCapturing / hipStreamEndCapture)"""
    try:
        hip = ctypes.CDLL("libamdhip64.so")
    except OSError:
        return
    for st in streams:
        status = ctypes.c_int(0)
        if hip.hipStreamIsCapturing(ctypes.c_void_p(st.cuda_stream), ctypes.byref(status)) == 0 and status.value != 0:
            graph = ctypes.c_void_p()
            hip.hipStreamEndCapture(ctypes.c_void_p(st.cuda_stream), ctypes.byref(graph))
            if graph.value:
                hip.hipGraphDestroy(graph)
    hip.hipGetLastError()     # (the sticky error of the failed capture is consumed here, not by the next launch)


def capture(stream, enqueue, other_streams=()):
    """capture what enqueue() launches on `stream` (and on `other_streams` it forks to) into a torch.cuda.CUDAGraph; nothing is executed.
    Returns (graph, None), or (None, the exception) when the capture failed; what is no Exception is raised again after the clean-up."""
    # (begin / end by hand instead of `with torch.cuda.graph(...)`: when the capture fails -- a collective that cannot be
    # captured -- the context manager's exit raises from capture_end() before it restores the current stream, and a stream
    # left capturing makes the next allocation or copy of the process fail.  Here a failed capture is ended, every stream
    # is checked, the current stream is restored, and the caller falls back to the eager enqueue.)
    g = torch.cuda.CUDAGraph()
    # no garbage collection inside the capture: a collected CUDAGraph of an env that went out of scope is DESTROYED by its finaliser,
    # hipGraphDestroy is not permitted while a stream captures, and the error thrown from that destructor ends the process
    # (seen once in the GPU suite under -s; torch.cuda.graph() collects before it captures for the same reason)
    gc.collect()
    torch.cuda.synchronize()
    gc_was_on = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.stream(stream):
            try:
                g.capture_begin(capture_error_mode="thread_local")
                enqueue()
                g.capture_end()
            except BaseException as exc:  # noqa: BLE001  (every failure takes this path: no exception type is exempt from the leak)
                try:
                    g.capture_end()
                except Exception:  # noqa: BLE001  (an invalidated capture reports its error again here)
                    pass
                _end_stray_capture((stream,) + tuple(other_streams))
                _never_destroy(g)
                if not isinstance(exc, Exception):
                    raise
                return None, exc
        return g, None
    finally:
        if gc_was_on:
            gc.enable()

"""What the context engines of libegoego_hip beside the denoiser share (stage1.Stage1Engine, stage1.FlowCNNEngine, body.BodyEngine):
one library context on one GPU with a grow-only workspace, and the engine cache of the nn.Modules in front of them.  The C side of
the same plumbing is csrc/host_util.h."""
import ctypes as C

import torch

from . import _lib


class ContextEngine:
    """One egoego_<mod>_ctx on one GPU.  A subclass names its module and the library's functions, creates the context with
    _create(...) and keeps its own load() and entry method."""

    NOUN = None  # "stage 1", "the flow CNN", ...: who "needs a cuda (ROCm) device"
    CREATE = DESTROY = WORKSPACE_BYTES = None  # names of the library's functions
    CHECK = None  # _lib.check_<mod>

    def __init__(self, device):
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.EgoEgoHipError(f"{self.NOUN} needs a cuda (ROCm) device; there is no CPU path")
        self.dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", self.dev_index)
        self._ctx = C.c_void_p()
        self._ws = None
        self._ws_home = None  # the stream self._ws was allocated under

    def _create(self, *args):
        type(self).CHECK(getattr(self.lib, self.CREATE)(*args, C.byref(self._ctx)))

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.dev_index).cuda_stream)

    def _workspace(self, *shape):
        """The workspace of a call of this shape on the current stream -> (pointer aligned to 256 bytes, bytes from there); the
        buffer only grows.  The caching allocator orders a freed block against the stream it was allocated under only: a buffer
        handed to the library under another stream is recorded on that stream, so that dropping it when it grows cannot give its
        memory to a later allocation while that stream still works in it."""
        n = getattr(self.lib, self.WORKSPACE_BYTES)(self._ctx, *shape)
        if n == 0:
            raise _lib.EgoEgoHipError(type(self).CHECK.last_error())
        return self._workspace_of(n)

    def _workspace_of(self, n):
        """_workspace for a byte count the caller already holds (a module without a context asks its own query)."""
        stream = torch.cuda.current_stream(self.dev_index)
        if self._ws is None or self._ws.numel() < n + 256:
            self._ws = torch.empty(n + 256, dtype=torch.uint8, device=self.device)
            self._ws_home = stream
        elif stream != self._ws_home:
            self._ws.record_stream(stream)
        off = (-self._ws.data_ptr()) % 256
        return self._ws.data_ptr() + off, self._ws.numel() - off

    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            getattr(self.lib, self.DESTROY)(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EngineCacheMixin:
    """For an nn.Module with `device`, `chunk_frames`, `_engine` and `_packed` (both None at first): to() remembers the device,
    engine() builds the engine anew when the device or the chunk changed and loads it again when the parameters did.  The
    module names its ENGINE class and gives _params_version() and _engine_state() (what the engine's load() takes)."""

    ENGINE = None

    def to(self, *args, **kwargs):
        """Moves the parameters like nn.Module.to and remembers the device the engine runs on (any form of the call: positional
        or keyword device, tensor, dtype only).  A CPU device makes engine() raise: there is no CPU path."""
        device = torch._C._nn._parse_to(*args, **kwargs)[0]
        if device is not None:
            self.device = torch.device(device)
        super().to(*args, **kwargs)
        return self

    def engine(self):
        dev = self.device
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        e = self._engine
        if e is None or e.device != dev or e.chunk_frames != self.chunk_frames:
            self._engine = self.ENGINE(dev, self.chunk_frames)
            self._packed = None
        v = self._params_version()
        if v != self._packed:
            self._engine.load(self._engine_state())
            self._packed = v
        return self._engine

"""Array backend of the nn framework on MI355X.

Mirrors the reference's backend switch `CP` (web_app/components/nn/gpu.py:5-29): `CP.cp`,
`CP.is_gpu_used`, `CP.use_gpu()`, `CP.copy(obj)` (host -> device), `CP.asnumpy(obj)` (device ->
host).  Where the reference binds `CP.cp` to CuPy and launches numba.cuda kernels, this backend
owns a `Runtime` (one per process = per GPU, with one `Lane` per context of libuniver_hip.so) and `DeviceArray`s
whose memory comes from PyTorch-ROCm's caching allocator (plumbing only: no torch op computes
anything on the hot path).

There is NO host compute path: `CP.use_cpu()` exists for API compatibility and raises, and every
op raises `HipError` when no MI355X is present.  Without a GPU, DeviceArrays can still be created
(storage-only, on the host) so that model construction, weight I/O and the data-parallel
bucketing logic are testable; any kernel call then fails loudly.
"""
import contextlib
import ctypes as C
import os

import numpy as np
# One hardware queue per stream (main, the PageTrainer lanes, copy / RCCL streams): ROCm's default of 4 per
# process makes streams share queues and run one after the other.  Read by the HIP runtime when it starts,
# i.e. at the first torch.cuda call after this import; an explicit setting in the environment wins.
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')

import torch

from ..hip import lib as hiplib
from ..hip.lib import HipError

_TORCH_DT = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64,
             np.dtype(np.float16): torch.float16,
             np.dtype(np.uint8): torch.uint8, np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64}
_CODE = {torch.float32: hiplib.F32, torch.float64: hiplib.F64, torch.float16: hiplib.F16}
_NP_DT = {v: k for k, v in _TORCH_DT.items()}


class Lane:
    """What belongs to one uocr_ctx of the library: the handle (null until Runtime._open has made the context), the torch
    stream its kernels go to, its side stream (a Lane of its own, made at the first Runtime.side on this lane) and the
    arrays held for its open deferred weight-gradient group (None: no group is open).
    A side Lane also has the events that order it with its lane (`fork_ev`, `join_ev`), the arrays its kernels read
    (`keep`, held until the join) and `dirty`: kernels have gone to it since the last join."""

    __slots__ = ('handle', 'stream', 'side', 'held', 'fork_ev', 'join_ev', 'keep', 'dirty')

    def __init__(self, stream=None, handle=None):
        self.handle = C.c_void_p() if handle is None else handle
        self.stream = stream
        self.side = self.held = self.fork_ev = self.join_ev = None
        self.keep, self.dirty = [], False


_NO_SCOPE = contextlib.nullcontext()


class Runtime:
    """The HIP contexts (stream + workspace each) of libuniver_hip.so in this process, one Lane per context; all kernels
    go through `call`, to the lane that is `current`.  Lane 0 is the main one: its stream is a dedicated torch stream made
    current, so torch's allocator, H2D/D2H copies, HIP-graph capture and RCCL collectives are ordered with the kernels."""

    def __init__(self, device_index=None):
        if not torch.cuda.is_available():
            raise HipError('no HIP device visible: the univer-ocr MI355X backend has no host fallback')
        if device_index is None:
            device_index = int(os.environ.get('LOCAL_RANK', '0')) % max(1, torch.cuda.device_count())
        self.device_index = device_index
        self.device = torch.device('cuda', device_index)
        torch.cuda.set_device(self.device)
        self.stream = self._stream()
        torch.cuda.set_stream(self.stream)
        main = Lane(self.stream)
        self._init_state(hiplib.get_lib(), main)
        self._open(main, f'main context on device {device_index}', int(os.environ.get('UOCR_WORKSPACE_MB', '256')) << 20)

    def _init_state(self, lib, main):
        """Everything but the device: `main` becomes lane 0 and the current one (its context need not exist yet)."""
        self.lib = lib
        self._fn = {}
        self.launches = 0
        self.lanes = [main]                          # lane 0 = the main stream
        self.current = main                          # the Lane `call` sends to; switched by `on` and by nothing else
        self.side_on = False                         # Model.backward turns it on for models with side_wgrad
        self.comm_lane = None                        # index of the communication lane (parallel.py), made on demand
        self._options = {}                           # what set_option has set, replayed on side streams made later

    @property
    def ctx(self):
        """The handle of the current lane (read only: `on` switches lanes)."""
        return self.current.handle

    def _stream(self, priority=0, external=None):
        """A new torch stream, or torch's wrapper of the stream `external` that the library made."""
        if external is not None:
            return torch.cuda.ExternalStream(external, device=self.device)
        return torch.cuda.Stream(device=self.device, priority=priority)   # -1 = high

    def _open(self, lane, what, workspace, cu_mask=None, options=False):
        """Make `lane`'s context, with `workspace` bytes: on its torch stream, or with cu_mask (words of CU bits) on a
        stream that the library creates on those CUs and torch merely wraps for its allocator's bookkeeping.  options:
        replay what set_option has set so far.  A context whose set-up fails is destroyed again."""
        if cu_mask is None:
            rc = self.lib.uocr_ctx_create(self.device_index, workspace, C.byref(lane.handle))
        else:
            rc = self.lib.uocr_ctx_create_cu_mask(self.device_index, workspace, cu_mask, len(cu_mask), C.byref(lane.handle))
        if rc != 0:
            raise HipError(f'uocr_ctx_create ({what}) failed with code {rc}')
        try:
            if cu_mask is not None:
                lane.stream = self._stream(external=self.lib.uocr_ctx_get_stream(lane.handle))
            with self.on(lane):
                if cu_mask is None:
                    self.call('uocr_ctx_set_stream', C.c_void_p(lane.stream.cuda_stream))
                for key, value in self._options.items() if options else ():
                    self.call('uocr_ctx_set_option', key.encode(), value)
        except BaseException as error:
            self.lib.uocr_ctx_destroy(lane.handle)
            lane.handle = C.c_void_p()
            if isinstance(error, HipError):
                raise HipError(f'{what}: {error}') from error
            raise
        return lane

    @contextlib.contextmanager
    def on(self, lane):
        """`with rt.on(lane):` -- `call` sends to `lane` inside and to the lane before it afterwards, however the block
        ends.  Switches the library's context only, not torch's current stream (`lane` does both)."""
        previous = self.current
        self.current = lane
        try:
            yield lane
        finally:
            self.current = previous

    # -- lanes: extra (context, stream) pairs so independent models run concurrently ---------------
    def add_lane(self, workspace_mb=256, priority=0, xcds=None):
        """A further HIP context of the library with its own stream and workspace; returns its index in `lanes`.  The
        four my_model nets are independent, so each trains on its own lane: the latency-bound kernels of the small
        nets run under the bandwidth-bound kernels of the large ones.
        xcds: an iterable of XCD numbers (0..7) -- the lane's stream is created by the library on those XCDs only.
        A new lane starts from the library's default options: what set_option set earlier is NOT replayed on it.
        Lanes are never released: every caller's lanes stay with the process-wide runtime."""
        if xcds is None:
            lane = self._open(Lane(self._stream(priority)), 'lane', int(workspace_mb) << 20)
        else:
            cus = self.device_info()['cu_count']
            mask = (C.c_uint32 * ((cus + 31) // 32))()
            for i in range(cus):
                if i % 8 in set(xcds):
                    mask[i // 32] |= 1 << (i % 32)
            lane = self._open(Lane(), f'lane on XCDs {sorted(set(xcds))}', int(workspace_mb) << 20, cu_mask=mask)
        self.lanes.append(lane)
        return len(self.lanes) - 1

    @contextlib.contextmanager
    def lane(self, index):
        """`with runtime.lane(i) as stream:` -- kernels, allocations and copies inside go to lane i's stream."""
        lane, previous = self.lanes[index], torch.cuda.current_stream()
        with self.on(lane):
            torch.cuda.set_stream(lane.stream)
            try:
                yield lane.stream
            finally:
                torch.cuda.set_stream(previous)

    def call(self, name, *args):
        fn = self._fn.get(name)
        if fn is None:
            fn = self._fn[name] = getattr(self.lib, name)
        rc = fn(self.current.handle, *args)
        self.launches += 1
        if rc != 0:
            msg = self.lib.uocr_last_error(self.current.handle)
            raise HipError(f'{name} failed ({rc}): {msg.decode() if msg else "?"}')

    def set_option(self, key, value):
        """Kernel selection knobs of the C ABI: 'mfma' (0 never / 1 auto / 2 whenever eligible),
        'fast_paths' (0 generic kernels only / 1 shape-specialised).  Applied to every lane, then to every side stream
        there is; recorded (for the side streams made later) once all of them have accepted it."""
        for lane in self.lanes + [lane.side for lane in self.lanes if lane.side is not None]:
            with self.on(lane):
                self.call('uocr_ctx_set_option', key.encode(), int(value))
        self._options[key] = int(value)

    def _report(self, symbol):
        """The values of the launch report `symbol` (a uocr_ctx_last_* getter) on the current lane: one out parameter per
        POINTER(T) that its prototype in hip.lib declares after the context."""
        outs = [pointer._type_() for pointer in hiplib._PROTOS[symbol][1:]]
        self.call(symbol, *[C.byref(out) for out in outs])
        return tuple(out.value for out in outs)

    def last_split(self):
        """(blocks, work items) of the most recent launch on the current lane whose split was decided at run time
        (persistent tile walks, rows or tiles per block: the launches the 'max_blocks' option lowers)."""
        return self._report('uocr_ctx_last_split')

    def last_gemm(self):
        """(row tile, row tiles, column tiles, depth slabs) of the most recent float32 MFMA GEMM on the current lane
        (uocr_ctx_last_gemm); a deferred weight-gradient group flush reports (64, 0, 0, its largest split)."""
        return self._report('uocr_ctx_last_gemm')

    def last_gemm_group(self):
        """(problems, split problems) of the most recent deferred weight-gradient group flush on the current lane."""
        return self._report('uocr_ctx_last_gemm_group')

    def last_pair(self):
        """(kernel, g, mode, pf, waves per block, blocks_x, bands, band_h) of the most recent Monochrome pair launch
        accepted on the current lane (uocr_ctx_last_pair): kernel 1 / 2 = float32 forward / backward, 3 = binary16
        forward, 4 / 5 = binary16 backward as one cooperative block / on independent waves; all 0 before the first."""
        return self._report('uocr_ctx_last_pair')

    def last_conv(self):
        """(entry, kernel) of the most recent uocr_conv2d_* call accepted on the current lane (uocr_ctx_last_conv): entry
        0 / 1 / 2 = forward / backward-data / backward-weight, kernel = a UOCR_CONV_* value (hip.lib.CONV_KERNELS names
        them); (0, 0) before the first."""
        return self._report('uocr_ctx_last_conv')

    def last_label(self):
        """(tile rows, tile columns, kernel launches) of the most recent uocr_label_components call on the current lane
        (uocr_ctx_last_label); all 0 before the first."""
        return self._report('uocr_ctx_last_label')

    def last_label_batch(self):
        """(tile rows, tile columns, entries per launch group, kernel launches) of the most recent uocr_label_batch call
        on the current lane (uocr_ctx_last_label_batch); all 0 before the first."""
        return self._report('uocr_ctx_last_label_batch')

    def last_char_label(self):
        """(columns per vote block, elements per statistics chunk, lines per launch, kernel launches) of the most recent
        uocr_char_label call on the current lane (uocr_ctx_last_char_label); all 0 before the first."""
        return self._report('uocr_ctx_last_char_label')

    def last_line_crop(self):
        """(output elements per block, bytes per vector store, entries per launch, kernel launches) of the most recent
        uocr_line_crop call on the current lane (uocr_ctx_last_line_crop); all 0 before the first."""
        return self._report('uocr_ctx_last_line_crop')

    def last_rotate(self):
        """(output rows per block of a probe, output pixels per block of an entry, probes / entries per launch, kernel
        launches) of the most recent uocr_rotated_extent or uocr_rotate_crop call on the current lane
        (uocr_ctx_last_rotate); all 0 before the first."""
        return self._report('uocr_ctx_last_rotate')

    def last_rotation_search(self):
        """(rounds, paragraphs per launch, kernel launches) of the most recent uocr_rotation_search call on the current
        lane (uocr_ctx_last_rotation_search); all 0 before the first."""
        return self._report('uocr_ctx_last_rotation_search')

    def last_pred_to_text(self):
        """(rows of a line per block, lines per launch, kernel launches) of the most recent uocr_pred_to_text call on the
        current lane (uocr_ctx_last_pred_to_text); all 0 before the first."""
        return self._report('uocr_ctx_last_pred_to_text')

    def last_pack_lines(self):
        """(elements of an entry per block at most, entries per launch, kernel launches) of the most recent uocr_pack_lines
        or uocr_zero_gaps call on the current lane (uocr_ctx_last_pack_lines); all 0 before the first."""
        return self._report('uocr_ctx_last_pack_lines')

    def last_page_gen(self):
        """(tile rows, tile columns, pages per launch, kernel launches) of the most recent uocr_page_layout or
        uocr_page_render call on the current lane (uocr_ctx_last_page_gen); all 0 before the first."""
        return self._report('uocr_ctx_last_page_gen')

    def set_loss_snapshot(self, arena):
        """From now on the fused optimizer tails launched on the CURRENT lane end by copying `arena`'s slots into the next
        row of its ring (LossArena.arm); None switches it off."""
        if arena is None:
            self.call('uocr_ctx_set_loss_snapshot', None, 0, None, 0, None)
        else:
            self.call('uocr_ctx_set_loss_snapshot', arena.array.ptr, arena.array.shape[0], arena.ring.ptr, arena.ring_len,
                      arena.counter.ptr)

    # -- deferred weight gradients (uocr_wgrad_defer_begin / _flush): one launch for the small GEMMs of a backward pass --
    @contextlib.contextmanager
    def defer_wgrad(self):
        """`with rt.defer_wgrad():` -- the weight-gradient GEMMs issued inside on the current lane that are too small
        to fill the chip are recorded by the library and run as ONE grid (+ one reduction) at the end of the block, or
        earlier at `flush_deferred()`.  The arrays they read are held until then (`keep`)."""
        lane = self.current
        if lane.held is not None:
            raise HipError('defer_wgrad: a deferred group is already open on this lane')
        self.call('uocr_wgrad_defer_begin')
        lane.held = held = []
        failed = True
        try:
            yield
            failed = False
        finally:
            lane.held = None
            try:
                self.call('uocr_wgrad_defer_flush', 0)
            except HipError:
                if not failed:
                    raise
            finally:
                held.clear()

    def keep(self, *arrays):
        """Hold `arrays` until the deferred weight gradients of the current lane have been flushed (no-op otherwise)."""
        held = self.current.held
        if held is not None:
            held.extend(arrays)

    def flush_deferred(self):
        """Run what has been recorded on the current lane now and keep recording (a gradient bucket is due)."""
        held = self.current.held
        if held is not None:
            self.call('uocr_wgrad_defer_flush', 1)
            held.clear()

    # -- side stream of a lane: kernels nobody waits for until the end of the backward pass (weight gradients) --------
    def side(self, *keep):
        """`with rt.side(x, dy):` -- the C-ABI calls inside go to the side stream of the current lane, ordered behind
        everything enqueued on the lane so far (device-side event); the lane does not wait for them until
        `join_side()`.  `keep`: the arrays the side kernels read -- held until the join so that the allocator cannot
        hand their memory to a later kernel of the lane.  No-op (the calls stay on the lane) unless `side_on`."""
        return self._fork_side(keep) if self.side_on else _NO_SCOPE

    @contextlib.contextmanager
    def _fork_side(self, keep):
        lane = self.current
        if lane.side is None:                        # its own uocr_ctx (stream + workspace), made at the first use
            side = Lane(self._stream())
            side.fork_ev, side.join_ev = Event(self), Event(self)
            lane.side = self._open(side, 'side stream', int(os.environ.get('UOCR_SIDE_WORKSPACE_MB', '128')) << 20,
                                   options=True)
        side = lane.side
        side.fork_ev.record()                        # on the lane
        with self.on(side):
            side.fork_ev.wait()                      # the side stream waits for the lane up to here
            side.keep.extend(keep)
            side.dirty = True
            yield

    def join_side(self):
        """The current lane waits (on the device) for its side stream."""
        side = self.current.side
        if side is None or not side.dirty:
            return
        with self.on(side):
            side.join_ev.record()
        side.join_ev.wait()
        side.dirty = False
        side.keep.clear()

    def synchronize(self):
        self.call('uocr_stream_sync')

    # -- events and HIP graphs of the C ABI (include/univer_hip.h) ------------------------------------------------
    def event(self):
        return Event(self)

    def capture(self, pool=None):
        """`with rt.capture(pool) as graph:` records the C-ABI calls made inside on the CURRENT ctx's stream into a
        HIP graph (uocr_graph_begin_capture / uocr_graph_end_capture); `graph.replay()` launches it on the ctx that
        is current then.  Arrays allocated inside come from `pool` (a torch.cuda.MemPool: memory only -- it keeps the
        graph's buffers away from every other allocation for as long as the pool lives)."""
        return _Capture(self, pool)

    def device_info(self):
        name = C.create_string_buffer(256)
        cus, hbm = C.c_int(), C.c_size_t()
        self.call('uocr_device_info', name, 256, C.byref(cus), C.byref(hbm))
        return {'name': name.value.decode(), 'cu_count': cus.value, 'hbm_bytes': hbm.value}


class Event:
    """HIP event of the C ABI: record() on the current ctx's stream, wait() = the current ctx's stream waits for it
    on the device, synchronize() = the host waits."""

    __slots__ = ('rt', 'handle')

    def __init__(self, rt):
        self.rt, self.handle = rt, C.c_void_p()
        if rt.lib.uocr_event_create(C.byref(self.handle)) != 0:
            raise HipError('uocr_event_create failed')

    def record(self):
        self.rt.call('uocr_event_record', self.handle)
        return self

    def wait(self):
        self.rt.call('uocr_stream_wait_event', self.handle)

    def synchronize(self):
        if self.rt.lib.uocr_event_synchronize(self.handle) != 0:
            raise HipError('uocr_event_synchronize failed')

    def __del__(self):
        try:
            if self.handle:
                self.rt.lib.uocr_event_destroy(self.handle)
        except Exception:   # noqa: BLE001  (interpreter shutdown)
            pass


class Graph:
    """An instantiated HIP graph of the C ABI; keeps its memory pool alive."""

    __slots__ = ('rt', 'handle', 'pool')

    def __init__(self, rt, handle, pool):
        self.rt, self.handle, self.pool = rt, handle, pool

    def replay(self):
        self.rt.call('uocr_graph_launch', self.handle)

    def __del__(self):
        try:
            if self.handle:
                self.rt.lib.uocr_graph_destroy(self.handle)
        except Exception:   # noqa: BLE001
            pass


class _Capture:
    def __init__(self, rt, pool):
        self.rt, self.pool, self.graph = rt, pool, None

    def __enter__(self):
        self._mem = torch.cuda.use_mem_pool(self.pool) if self.pool is not None else None
        if self._mem is not None:
            self._mem.__enter__()
        torch.cuda.synchronize()
        self.rt.call('uocr_graph_begin_capture')
        self.graph = Graph(self.rt, None, self.pool)
        return self.graph

    def __exit__(self, exc_type, exc, tb):
        handle = C.c_void_p()
        try:
            self.rt.join_side()                      # a forked side stream must be back before the capture ends
            self.rt.call('uocr_graph_end_capture', C.byref(handle))
            self.graph.handle = handle
        except HipError:
            if exc_type is None:
                raise
        finally:
            if self._mem is not None:
                self._mem.__exit__(exc_type, exc, tb)
        return False


class LossArena:
    """Consecutive float64 loss slots in ONE device array: the loss kernels of a captured step write side by side.
    Per-step snapshots: `arm()` gives the arena a ring of `ring_len` rows; with Runtime.set_loss_snapshot(arena) in force
    the step's last kernel (the fused optimizer tail) copies the slots into the next row by itself
    (uocr_ctx_set_loss_snapshot), and `next_row()` names that row on the host -- no copy launch.  A row is overwritten
    `ring_len` steps later: a DeviceScalar made from a row with `arena=` remembers `rows` and refuses to be read for the
    first time once `ring_len` further tails have been launched (a HipError, never another step's number).  The host's
    `rows` and the device counter agree as long as every tail launched with this arena's snapshot in force is followed by
    one `next_row()`; tails launched with the snapshot off (eager steps of a captured net) advance neither."""

    def __init__(self, capacity=16, ring_len=64):
        if int(ring_len) < 1:
            raise HipError(f'LossArena: ring_len {ring_len} < 1')
        self.array = CP.empty((capacity,), np.float64)
        self.used = 0
        self.ring_len = int(ring_len)
        self.ring = self.counter = None
        self.rows = 0                                # optimizer tails launched since arm() (the device counts the same)

    def take(self):
        if self.used >= self.array.shape[0]:
            raise HipError('loss arena full')
        slot = DeviceArray(self.array.t[self.used:self.used + 1])
        self.used += 1
        return slot

    def index_of(self, tensor):
        return (tensor.data_ptr() - self.array.ptr) // 8

    def snapshot(self):
        """a copy of the used slots, made on the current ctx's stream (one uocr_d2d)"""
        out = CP.empty((self.used,), np.float64)
        CP.runtime().call('uocr_d2d', out.ptr, self.array.ptr, 8 * self.used)
        return out

    def arm(self):
        """allocate the ring and its device counter (not inside a graph capture: the counter is zeroed once)"""
        capacity = self.array.shape[0]
        self.ring = CP.empty((self.ring_len * capacity,), np.float64)
        self.counter = CP.zeros((1,), np.int32)
        self.rows = 0
        return self

    def next_row(self):
        """the ring row the optimizer tail that was just launched writes: a view, valid until ring_len further tails have
        been launched (DeviceScalar(row.t[i], arena=self), made before the next call, enforces that)"""
        capacity = self.array.shape[0]
        k = self.rows % self.ring_len
        self.rows += 1
        return DeviceArray(self.ring.t[k * capacity:(k + 1) * capacity])


class DeviceArray:
    """N-d C-contiguous array in HBM (NHWC for images).  Only what the framework needs: shape /
    dtype / reshape (a view) / copy / host round trip / `+` for fan-out gradient sums
    (models.py:218).  All arithmetic happens in libuniver_hip.so."""

    __slots__ = ('t', 'gscale')
    __array_priority__ = 100

    def __init__(self, tensor, gscale=0):
        self.t = tensor
        # float16 mode: log2 of the power-of-two factor this array carries when it is an activation GRADIENT
        # (set by the loss kernels, handed on by every backward op, removed by the bwd_weight kernels:
        # include/univer_hip.h, UOCR_F16_SCALED).  0 for everything else.
        self.gscale = gscale

    # -- metadata ---------------------------------------------------------------------------
    @property
    def shape(self):
        return tuple(self.t.shape)

    @property
    def dtype(self):
        return _NP_DT[self.t.dtype]

    @property
    def size(self):
        return self.t.numel()

    @property
    def ndim(self):
        return self.t.dim()

    @property
    def nbytes(self):
        return self.t.numel() * self.t.element_size()

    @property
    def ptr(self):
        return self.t.data_ptr()

    @property
    def code(self):
        code = _CODE.get(self.t.dtype)
        if code is None:
            raise HipError(f'{self.t.dtype} arrays have no kernel dtype code')
        return code | (self.gscale << 8) if code == hiplib.F16 else code

    def __len__(self):
        return self.t.shape[0]

    def __repr__(self):
        return f'DeviceArray(shape={self.shape}, dtype={self.dtype}, device={self.t.device})'

    # -- views / copies -----------------------------------------------------------------------
    def reshape(self, *shape):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list)):
            shape = tuple(shape[0])
        return DeviceArray(self.t.view(*[int(s) for s in shape]), self.gscale)

    def copy(self):
        return DeviceArray(self.t.clone(), self.gscale)

    def numpy(self):
        return self.t.detach().cpu().numpy()

    def __array__(self, dtype=None, copy=None):
        a = self.numpy()
        return a if dtype is None else a.astype(dtype, copy=False)

    def tolist(self):
        return self.numpy().tolist()

    def set(self, host):
        """Overwrite the contents with a host array of the same shape (keeps the storage)."""
        host = np.ascontiguousarray(host, dtype=self.dtype)
        if host.shape != self.shape:
            raise ValueError(f'shape mismatch: {host.shape} != {self.shape}')
        self.t.copy_(torch.from_numpy(host))
        return self

    def __add__(self, other):
        if isinstance(other, (int, float)) and other == 0:
            return self
        if not isinstance(other, DeviceArray):
            return NotImplemented
        return CP.ops.add(self, other)

    __radd__ = __add__


class _Random:
    """CP.cp.random.* of the test scripts (test_gradients.py:65-70): host RNG, then H2D."""

    @staticmethod
    def randn(*shape):
        return CP.copy(np.random.randn(*shape))

    @staticmethod
    def rand(*shape):
        return CP.copy(np.random.rand(*shape))

    @staticmethod
    def uniform(low=0.0, high=1.0, size=None):
        return CP.copy(np.random.uniform(low, high, size))


class _ArrayModule:
    """The slice of the NumPy/CuPy module API the framework and its test scripts use on `CP.cp`."""
    random = _Random()
    ndarray = DeviceArray

    @staticmethod
    def zeros(shape, dtype=None):
        return CP.zeros(shape, dtype)

    @staticmethod
    def ones(shape, dtype=None):
        return CP.full(shape, 1.0, dtype)

    @staticmethod
    def zeros_like(a):
        return CP.zeros(a.shape, a.dtype)

    @staticmethod
    def array(obj, dtype=None):
        return CP.copy(obj, dtype)

    asarray = array

    @staticmethod
    def reshape(a, shape):
        return a.reshape(shape)

    @staticmethod
    def copy(a):
        return a.copy()


class CP:
    """Backend switch with the reference's interface (nn/gpu.py:5-29)."""
    cp = _ArrayModule()
    is_gpu_used = True
    dtype = np.dtype(os.environ.get('UOCR_DTYPE', 'float32'))
    lazy_losses = False          # True: losses stay on the device until float() is called
    loss_arena = None            # a LossArena: loss slots come from it (graph capture, my_model/trainer.py)
    f16_grad_scale_log2 = None   # float16 mode: None = the loss kernels pick the gradient scale, int k = 2^k
    _runtime = None
    ops = None                   # set by nn/ops.py (kernel wrappers)

    @staticmethod
    def use_cpu():
        raise NotImplementedError(
            'CP.use_cpu(): the MI355X backend ships no host compute path. The NumPy mode of the '
            'reference (nn/gpu.py:9-12) is the reference itself; tests compare against oracle/.')

    @staticmethod
    def use_gpu(device_index=None):
        CP.is_gpu_used = True
        CP.runtime(device_index)

    @staticmethod
    def set_dtype(dtype):
        """float32 (production), float64 (the reference's type: parity mode) or float16 = binary16 ACTIVATIONS
        with float32 parameters / gradients / accumulation (BASELINE configs[4], include/univer_hip.h UOCR_F16)."""
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.float32), np.dtype(np.float64), np.dtype(np.float16)):
            raise HipError(f'unsupported compute dtype {dt}')
        CP.dtype = dt

    @staticmethod
    def param_dtype():
        """dtype of parameters, their gradients and optimizer state: float32 master copies in float16 mode."""
        return np.dtype(np.float32) if CP.dtype == np.dtype(np.float16) else CP.dtype

    @staticmethod
    def runtime(device_index=None):
        if CP._runtime is None:
            CP._runtime = Runtime(device_index)
        return CP._runtime

    @staticmethod
    def has_device():
        return torch.cuda.is_available()

    @staticmethod
    def storage_device():
        if CP._runtime is not None:
            return CP._runtime.device
        if torch.cuda.is_available():
            return CP.runtime().device
        return torch.device('cpu')      # storage-only mode (no kernels can run)

    @staticmethod
    def loss_slot():
        """one float64 device slot a loss / regularisation kernel writes its value to"""
        if CP.loss_arena is not None:
            return CP.loss_arena.take()
        return CP.empty((1,), np.float64)

    # -- allocation -----------------------------------------------------------------------------
    @staticmethod
    def empty(shape, dtype=None):
        dt = CP.dtype if dtype is None else np.dtype(dtype)
        shape = (shape,) if isinstance(shape, (int, np.integer)) else tuple(int(s) for s in shape)
        return DeviceArray(torch.empty(shape, dtype=_TORCH_DT[dt], device=CP.storage_device()))

    @staticmethod
    def zeros(shape, dtype=None):
        """cupy.zeros: allocation (torch's caching allocator) + uocr_memset_zero -- no torch kernel runs."""
        out = CP.empty(shape, dtype)
        if out.t.is_cuda:
            if out.size:
                CP.runtime().call('uocr_memset_zero', out.ptr, out.nbytes)
        else:
            out.t.zero_()                   # storage-only mode (no GPU): host memory
        return out

    @staticmethod
    def full(shape, value, dtype=None):
        out = CP.empty(shape, dtype)
        if out.t.is_cuda and out.t.dtype in _CODE:
            if out.size:
                CP.runtime().call('uocr_fill', _CODE[out.t.dtype], out.ptr, float(value), out.size)
        else:
            out.t.fill_(value)
        return out

    # -- host <-> device (gpu.py:19-29) ------------------------------------------------------------
    @staticmethod
    def copy(obj, dtype=None):
        """Host array (or DeviceArray) -> new DeviceArray in the compute dtype."""
        dt = CP.dtype if dtype is None else np.dtype(dtype)
        if isinstance(obj, DeviceArray):
            if obj.dtype == dt:
                return obj.copy()
            return DeviceArray(obj.t.to(_TORCH_DT[dt]))
        host = np.ascontiguousarray(np.asarray(obj), dtype=dt)
        return DeviceArray(torch.from_numpy(host).to(CP.storage_device()))

    @staticmethod
    def asnumpy(obj):
        if isinstance(obj, DeviceArray):
            return obj.numpy()
        return np.asarray(obj)


class DeviceScalar:
    """A float64 loss value that lives in a device slot until somebody needs the number.  The
    reference converts every loss with float() right away (losses.py:25,42,57,73 -- one host sync
    each); with CP.lazy_losses the sync happens once, when the caller formats / adds the value.
    `arena`: the slot is in the row LossArena.next_row() has just named; the first read fails once the ring has come
    round to that row again (a host-side comparison of two counts: no device work)."""

    __slots__ = ('t', '_value', 'ready', 'arena', 'stamp')

    def __init__(self, tensor, ready=None, arena=None):
        self.t = tensor          # 0-d or 1-element float64 tensor
        self._value = None
        self.ready = ready       # event of the stream that writes the slot, when that is not the reader's stream
        self.arena = arena       # the LossArena whose ring row holds the slot, or None
        self.stamp = arena.rows if arena is not None else 0      # tails launched up to and including this value's own

    def __float__(self):
        if self._value is None:
            if self.arena is not None and self.arena.rows - self.stamp >= self.arena.ring_len:
                raise HipError(f'loss read {self.arena.rows - self.stamp} steps after its own: its row of the snapshot ring '
                               f'has been overwritten (snapshot_ring_len = {self.arena.ring_len}); read losses within '
                               f'snapshot_ring_len steps or raise PageTrainer(snapshot_ring_len=...)')
            if self.ready is not None:
                self.ready.synchronize()
            self._value = float(self.t.item())
        return self._value

    def __add__(self, other):
        return float(self) + float(other)

    __radd__ = __add__

    def __sub__(self, other):
        return float(self) - float(other)

    def __rsub__(self, other):
        return float(other) - float(self)

    def __mul__(self, other):
        return float(self) * float(other)

    __rmul__ = __mul__

    def __truediv__(self, other):
        return float(self) / float(other)

    def __lt__(self, other):
        return float(self) < float(other)

    def __gt__(self, other):
        return float(self) > float(other)

    def __format__(self, spec):
        return format(float(self), spec)

    def __repr__(self):
        return repr(float(self))

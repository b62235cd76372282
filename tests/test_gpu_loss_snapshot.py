"""Loss snapshots (uocr_ctx_set_loss_snapshot): the ring rows the fused optimizer tails write, on every exit path of
opt_fused_kernel, past one lap of the ring, through a replayed graph and through PageTrainer.

With a snapshot configured the fused Momentum / Adam tail ends by copying the ctx's loss slots into row
(device counter mod ring_len) of a ring.  The regularisation loss the same kernel stores is usually one of those
slots (the trainer's arena: the LAST one), so the row must hold the value stored by THAT call.  The kernel calls the
copy from three places: without ranges (block 0, while other blocks may still run), with ranges in one block, with
ranges in several blocks (the last block to arrive, after the sum inside the launch).

| test | what it pins |
|---|---|
| ring_rows_through_the_abi | K = 2 ring_len + 1 calls (ring_len + 3 at 64) without a host sync in between, slots that encode the call number exactly and a regularisation loss that differs by more than 1000 x the tolerance from call to call: every row holds the slots of the last call mapped to it bit for bit, its regularisation entry is the oracle's (float64 on the stored weights) within 1e-5 / 1e-12 and bit-equal to what the same calls return with the snapshot off; sentinel rows, the counter (= K), w / v / a against the run with the snapshot off |
| off_on_and_empty_calls | slots == NULL: neither ring nor counter move; configured again the numbering continues; rows never reached stay NaN; a call with count == 0 parameters launches nothing (launch_opt_fused returns before the launch: today's behaviour, pinned) and so writes no row; the argument refusals |
| captured_step_replayed | one graph of softmax CE, sigmoid CE, Dice and a fused Momentum tail -- the kernels that hand partial sums to each other through the ctx's sync words and workspace -- replayed 8 times over a ring of 3 |
| trainer_past_one_lap | PageTrainer(graphs=True, pipelined=True, snapshot_ring_len=4 / 64) for ring_len + 6 steps with two eager steps of the Line net in between: late reads of the last ring_len steps are the per-step truth, older ones raise, host and device counts agree |

References: oracle/nn_oracle.py in float64 on the inputs rounded to the storage type, or exact copying.  Tolerances
are the project's (test_gpu_streaming_ops.py, whose helpers this file uses).  The tests without the `gpu` mark check
the seeds (the regularisation losses of consecutive calls are far enough apart for an off-by-one row to fail), the
host-side staleness guard of DeviceScalar and the refusal of a null ctx.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import nn_oracle as O
from test_gpu_streaming_ops import (TOL, Buf, cdiv, close, fused_ranges, gpu, loss_close, rs, same_bits,  # noqa: F401
                                    seg_inputs, wanted_blocks)

# (n, ranges?, exit path of opt_fused_kernel)
SNAP_SIZES = [
    (5, False, 'no ranges, one block'),
    (5003, False, 'no ranges, several blocks'),
    (5, True, 'ranges, one block'),
    (5003, True, 'ranges, last block to arrive'),
    (300001, True, 'ranges, capped grid'),
]
RINGS = [(1, 1), (5, 3), (16, 64)]                # (count, ring_len)
HYPER = {'momentum': (0.05, 0.9), 'adam': (0.0015, 0.9, 0.999, O.EPS_OPT)}


def calls_for(ring_len):
    return ring_len + 3 if ring_len == 64 else 2 * ring_len + 1


def snap_ranges(n):
    """four ranges as in test_gpu_streaming_ops.fused_ranges (one of them empty); n = 5: two elements, one, none, two"""
    if n >= 2049:
        return fused_ranges(n, False)
    return [(('l2', 2.0 ** -7), 0, 2), (('l1', 3 * 2.0 ** -8), 2, 3), (('l2', 2.0 ** -8), 3, 3), (('l1', 2.0 ** -6), n - 2, n)]


def call_scale(k):
    """the weights of call k are one base vector times this: 0.5 .. 1.6, steps of 3/8 or 5/8 between consecutive calls"""
    return 0.5 + ((5 * k) % 8) / 8 + k / 1024


def snap_base(n, dtype):
    """base weights (no element closer to zero than 0.25), three gradients, velocity, accumulated squares"""
    rng = np.random.default_rng(7 * n + np.dtype(dtype).itemsize)
    base = rng.uniform(0.25, 1.5, n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    grads = [rs(rng.standard_normal(n), dtype) for _ in range(3)]
    return base, grads, rs(rng.standard_normal(n) * 0.1, dtype), rs(rng.uniform(1e-3, 1.0, n), dtype)


def weights_of_call(base, k, dtype):
    return rs(base * call_scale(k), dtype)


def oracle_reg_loss(w, ranges):
    """the loss part of test_gpu_streaming_ops.oracle_fused: O.l1_reg / O.l2_reg on each range of the stored weights"""
    return float(sum((O.l1_reg if kind == 'l1' else O.l2_reg)(w[lo:hi], strength)[0] for (kind, strength), lo, hi in ranges))


def slot_values(k, count):
    """exact in float64, different for every (call, slot)"""
    return k + np.arange(count) / 64.0


def range_args(ranges):
    n = len(ranges)
    return (n, (C.c_longlong * max(n, 1))(*[r[1] for r in ranges]), (C.c_longlong * max(n, 1))(*[r[2] for r in ranges]),
            (C.c_int * max(n, 1))(*[{'l1': 1, 'l2': 2}[r[0][0]] for r in ranges]),
            (C.c_double * max(n, 1))(*[float(r[0][1]) for r in ranges]))


def fused_call(rt, opt, w, g, v, a, n, ranges, reg_ptr):
    """one fused tail through the C ABI (zero_grad on, hyper-parameters by value)"""
    if opt == 'momentum':
        rt.call('uocr_momentum_step_fused', w.v.code, w.v.ptr, g.v.ptr, v.v.ptr, n, *HYPER[opt], *range_args(ranges), reg_ptr,
                1, None)
    else:
        rt.call('uocr_adam_step_fused', w.v.code, w.v.ptr, g.v.ptr, v.v.ptr, a.v.ptr, n, *HYPER[opt], *range_args(ranges),
                reg_ptr, 1, None)


class Counter:
    """one device word between two sentinel words"""

    def __init__(self, CP):
        self.CP = CP
        self.base = CP.copy(np.array([-7, 0, -7], np.int32), np.int32)
        self.ptr = self.base.ptr + 4

    def get(self):
        host = self.CP.asnumpy(self.base)
        assert host[0] == -7 and host[2] == -7, 'wrote next to the counter'
        return int(host[1])


# ---- without a GPU ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_seeds_keep_consecutive_regularisation_losses_apart(dtype):
    """What makes the bit-equality of a row's regularisation entry with "the same call, snapshot off" a test of WHICH
    call the row holds: on the oracle alone, the regularisation loss of call k differs from that of call k - 1, and of
    the call that wrote the row one lap earlier, by more than 1000 x TOL relative -- for every size with ranges."""
    for n, with_ranges, _ in SNAP_SIZES:
        if not with_ranges:
            continue
        base = snap_base(n, dtype)[0]
        ranges = snap_ranges(n)
        losses = [oracle_reg_loss(weights_of_call(base, k, dtype), ranges) for k in range(calls_for(64))]
        assert min(losses) > 0
        for back in (1, 3, 64):
            for k in range(back, len(losses)):
                gap = abs(losses[k] - losses[k - back]) / max(losses[k], losses[k - back])
                assert gap > 1000 * TOL[dtype], f'n={n} {dtype}: calls {k - back} and {k} are only {gap:.2e} apart'


def test_a_recycled_row_refuses_to_be_read():
    """DeviceScalar(row.t[i], arena=arena): the first read raises once ring_len further rows have been handed out (host
    arithmetic on LossArena.rows, nothing on the device); a value read in time stays cached; next_row() walks the ring."""
    from univer_ocr_amd.hip import HipError
    from univer_ocr_amd.nn.gpu import DeviceScalar, LossArena
    arena = LossArena(4, ring_len=3).arm()
    arena.ring.t.zero_()
    kept, early = [], None
    for step in range(5):
        row = arena.next_row()
        assert arena.rows == step + 1
        assert row.ptr == arena.ring.ptr + (step % 3) * 4 * 8 and row.shape == (4,)
        row.t[1] = 10.0 + step                                   # what the step's last kernel would do
        kept.append(DeviceScalar(row.t[1], arena=arena))
        if step == 0:
            early = DeviceScalar(row.t[1], arena=arena)
            assert float(early) == 10.0
    assert float(early) == 10.0                                  # read in time: cached, although its row now holds step 3
    for step, value in enumerate(kept):
        if step < 2:
            with pytest.raises(HipError, match=rf'{5 - (step + 1)} steps .*snapshot_ring_len = 3'):
                float(value)
            with pytest.raises(HipError):                        # ... and again: nothing was cached
                value + 1.0
        else:
            assert float(value) == 10.0 + step
    assert float(DeviceScalar(arena.ring.t[1])) == 13.0          # without an arena: the plain slot, as before
    with pytest.raises(HipError):
        LossArena(4, ring_len=0)


def test_set_loss_snapshot_refuses_a_null_ctx():
    from univer_ocr_amd.hip import lib as hiplib
    lib = hiplib.get_lib()
    assert lib.uocr_ctx_set_loss_snapshot(None, None, 0, None, 0, None) != 0


def test_snapshot_ring_len_defaults_to_64():
    import inspect

    from univer_ocr_amd.my_model.trainer import PageTrainer
    assert inspect.signature(PageTrainer.__init__).parameters['snapshot_ring_len'].default == 64


# ---- a. ring rows through the ABI ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('reg', ['last-slot', 'own-array'])
@pytest.mark.parametrize('ring', RINGS, ids=lambda r: f'{r[0]}x{r[1]}')
@pytest.mark.parametrize('size', range(len(SNAP_SIZES)),
                         ids=lambda i: f'n{SNAP_SIZES[i][0]}-{"ranges" if SNAP_SIZES[i][1] else "plain"}')
@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('opt', ['momentum', 'adam'])
def test_ring_rows_through_the_abi(opt, dtype, off, size, ring, reg, gpu):  # noqa: F811
    CP = gpu(dtype)
    rt = CP.runtime()
    tol = TOL[dtype]
    n, with_ranges, path = SNAP_SIZES[size]
    count, ring_len = ring
    K = calls_for(ring_len)
    ranges = snap_ranges(n) if with_ranges else []
    blocks = wanted_blocks(n if off else cdiv(n, 4))
    if 'one block' in path:
        assert blocks == 1
    elif 'capped' in path:
        assert blocks > 256                                      # OPT_FUSED_REG_GRID (launch_opt_fused)
    else:
        assert 1 < blocks <= 256
    tag = f'{opt} {dtype} n={n} off={off} {path}, {count} slots x {ring_len} rows, loss to {reg}'
    base, grads, v0, a0 = snap_base(n, dtype)
    w_host = np.stack([weights_of_call(base, k, dtype) for k in range(K)])
    slot_host = np.stack([slot_values(k, count) for k in range(K)])
    w_all, g_all, slot_all = CP.copy(w_host, dtype), CP.copy(np.stack(grads), dtype), CP.copy(slot_host, np.float64)
    item = np.dtype(dtype).itemsize

    def run(snapshot):
        w, g, v, a = Buf(CP, n, dtype, off), Buf(CP, n, dtype, off), Buf(CP, n, dtype, off, v0), Buf(CP, n, dtype, off, a0)
        slots, own = Buf(CP, count, 'float64'), Buf(CP, 1, 'float64')
        ring_buf, counter = Buf(CP, ring_len * count, 'float64'), Counter(CP)
        reg_ptr = slots.v.ptr + 8 * (count - 1) if reg == 'last-slot' else own.v.ptr
        losses = []
        if snapshot:
            rt.call('uocr_ctx_set_loss_snapshot', slots.v.ptr, count, ring_buf.v.ptr, ring_len, counter.ptr)
        try:
            for k in range(K):                                   # (no host sync in here when the snapshot is on)
                rt.call('uocr_d2d', w.v.ptr, w_all.ptr + k * n * item, n * item)
                rt.call('uocr_d2d', g.v.ptr, g_all.ptr + (k % 3) * n * item, n * item)
                rt.call('uocr_d2d', slots.v.ptr, slot_all.ptr + k * count * 8, count * 8)
                fused_call(rt, opt, w, g, v, a, n, ranges, reg_ptr)
                if not snapshot:
                    losses.append(float((slots.get(tag)[-1:] if reg == 'last-slot' else own.get(tag))[0]))
        finally:
            rt.call('uocr_ctx_set_loss_snapshot', None, 0, None, 0, None)
        return dict(w=w.get(tag), g=g.get(tag), v=v.get(tag), a=a.get(tag), slots=slots.get(tag), own=own.get(tag),
                    ring=ring_buf.get(tag + ' ring').reshape(ring_len, count), counter=counter.get(), losses=losses)

    plain, snap = run(False), run(True)
    assert snap['counter'] == K and plain['counter'] == 0, f'{tag}: counter {snap["counter"]} after {K} calls'
    assert np.isnan(plain['ring']).all(), tag + ': ring written with the snapshot off'
    for name in ('w', 'v', 'a', 'slots', 'own'):
        same_bits(snap[name], plain[name], f'{tag}: {name} with the snapshot on vs off')
    assert not np.any(snap['g']), tag + ': gradient not reset'
    ref_losses = [oracle_reg_loss(w_host[k], ranges) for k in range(K)]
    for k in range(K):                                           # the plain run itself against the oracle
        if ranges:
            loss_close(plain['losses'][k], ref_losses[k], tol, f'{tag}, call {k}, snapshot off')
        elif reg == 'last-slot':                                 # no ranges: reg_loss_out is not written at all
            assert plain['losses'][k] == slot_host[k, -1]
        else:
            assert np.isnan(plain['losses'][k])
    for r in range(ring_len):
        mapped = [k for k in range(K) if k % ring_len == r]
        row = snap['ring'][r]
        if not mapped:
            assert np.isnan(row).all(), f'{tag}: row {r} was never reached but holds {row}'
            continue
        k = mapped[-1]
        expected = slot_host[k].copy()
        if ranges and reg == 'last-slot':
            loss_close(row[-1], ref_losses[k], tol, f'{tag}: row {r}, regularisation loss of call {k}')
            expected[-1] = plain['losses'][k]                    # bit for bit the loss of call k, not of k - 1 or k - ring_len
        same_bits(row, expected, f'{tag}: row {r} = slots of call {k}')
    if ranges and reg == 'own-array':
        assert float(snap['own'][0]) == plain['losses'][-1]


# ---- b. off, on, empty calls, refusals ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('opt', ['momentum', 'adam'])
def test_off_on_and_empty_calls(opt, gpu):  # noqa: F811
    """launch_opt_fused returns before the launch when count == 0, so such a call writes no row and leaves the counter
    alone: pinned here as today's behaviour (LossArena.next_row must not be called for it either)."""
    from univer_ocr_amd.hip import HipError
    dtype, n, count, ring_len = 'float32', 5003, 4, 5
    CP = gpu(dtype)
    rt = CP.runtime()
    ranges = snap_ranges(n)
    base, grads, v0, a0 = snap_base(n, dtype)
    w, g, v, a = Buf(CP, n, dtype), Buf(CP, n, dtype), Buf(CP, n, dtype, 0, v0), Buf(CP, n, dtype, 0, a0)
    slots, ring_buf, counter = Buf(CP, count, 'float64'), Buf(CP, ring_len * count, 'float64'), Counter(CP)
    reg_ptr = slots.v.ptr + 8 * (count - 1)
    made = []                                                    # (call number, its regularisation loss) in issue order

    def call(size=n, rr=ranges):
        k = len(made)
        w.v.set(weights_of_call(base, k, dtype))
        g.v.set(grads[k % 3])
        slots.v.set(slot_values(k, count))
        fused_call(rt, opt, w, g, v, a, size, rr, reg_ptr)
        made.append(float(slots.get('slots')[-1]))
        return k

    def state():
        return ring_buf.get('ring').reshape(ring_len, count), counter.get()

    def configure():
        rt.call('uocr_ctx_set_loss_snapshot', slots.v.ptr, count, ring_buf.v.ptr, ring_len, counter.ptr)

    def check_row(row, k):
        loss_close(row[-1], oracle_reg_loss(weights_of_call(base, k, dtype), ranges), TOL[dtype], f'{opt}: row of call {k}')
        same_bits(row, np.append(slot_values(k, count)[:-1], made[k]), f'{opt}: row of call {k}')

    try:
        configure()
        first = [call(), call()]
        rows, cnt = state()
        assert cnt == 2 and np.isnan(rows[2:]).all()
        rt.call('uocr_ctx_set_loss_snapshot', None, 0, None, 0, None)          # off: nothing moves
        call(), call()
        after, cnt = state()
        same_bits(after, rows, f'{opt}: ring with the snapshot off')
        assert cnt == 2
        rt.call('uocr_ctx_set_loss_snapshot', None, 7, ring_buf.v.ptr, -1, None)   # off whatever else is passed
        call()
        assert state()[1] == 2
        configure()                                              # on again: the numbering goes on at the counter
        empty = [call(0, []), call(0, [(('l2', 0.5), 0, 0)])]    # no parameters: no launch, no row
        after, cnt = state()
        same_bits(after, rows, f'{opt}: ring after calls with count == 0')
        assert cnt == 2 and made[empty[0]] == slot_values(empty[0], count)[-1]
        sp, rp, cp = slots.v.ptr, ring_buf.v.ptr, counter.ptr
        for bad in ((sp, 0, rp, ring_len, cp), (sp, -1, rp, ring_len, cp), (sp, count, None, ring_len, cp),
                    (sp, count, rp, 0, cp), (sp, count, rp, -3, cp), (sp, count, rp, ring_len, None)):
            with pytest.raises(HipError, match='bad argument'):
                rt.call('uocr_ctx_set_loss_snapshot', *bad)
        second = [call(), call()]                                # (a refused call leaves the configuration as it was)
        rows, cnt = state()
        assert cnt == 4
        for r, k in enumerate(first + second):
            check_row(rows[r], k)
        assert np.isnan(rows[4]).all(), 'row 4 was never reached'
        third = [call(), call()]                                 # across the end of the ring: rows 4 and 0
        rows, cnt = state()
        assert cnt == 6
        for r, k in ((4, third[0]), (0, third[1]), (1, first[1]), (2, second[0]), (3, second[1])):
            check_row(rows[r], k)
    finally:
        rt.call('uocr_ctx_set_loss_snapshot', None, 0, None, 0, None)


# ---- c. a captured step replayed -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_captured_step_replayed():
    """Softmax CE, sigmoid CE, Dice and a fused Momentum tail with ranges (5 blocks: the last block to arrive sums
    up) back to back in ONE graph: each of them ends in a hand-over through the ctx's sync words / workspace, the tail
    snapshots the four slots.  8 replays over a ring of 3, new inputs and weights before each."""
    import torch

    from univer_ocr_amd.nn import CP, ops
    from univer_ocr_amd.nn.gpu import LossArena
    CP.use_gpu(0)
    CP.set_dtype('float32')
    rt = CP.runtime()
    dtype, n, ring_len, replays = 'float32', 5003, 3, 2 * 3 + 2
    ranges = snap_ranges(n)
    assert 1 < wanted_blocks(cdiv(n, 4)) <= 256
    base, grads, v0, _ = snap_base(n, dtype)

    def batch(j):
        rng = np.random.default_rng(100 + j)
        sm_pred = rs(rng.standard_normal((37, 10)) * 3.0, dtype)
        sm_gt = np.zeros((37, 10))
        sm_gt[np.arange(37), rng.integers(0, 10, 37)] = 1.0
        sg_pred = rs(np.clip(rng.standard_normal((300, 1)) * 4.0, -12.0, 12.0), dtype)
        sg_gt = (rng.random((300, 1)) > 0.7).astype(np.float64)
        dice_pred, dice_gt = seg_inputs(rng, (1, 16, 24, 1), dtype)
        return [sm_pred, sm_gt, sg_pred, sg_gt, dice_pred, dice_gt, weights_of_call(base, j, dtype), grads[j % 3]]

    def oracle(b):
        return [O.softmax_ce_loss(b[0], b[1])[0], O.sigmoid_ce_loss(b[2], b[3])[0], O.dice_loss(b[4], b[5])[0],
                oracle_reg_loss(b[6], ranges)]

    def step(s, v):
        return [ops.softmax_ce(s[0], s[1])[0], ops.sigmoid_ce(s[2], s[3])[0], ops.seg_loss('dice', s[4], s[5])[0],
                ops.momentum_step_fused(s[6], s[7], v, *HYPER['momentum'], ranges)]

    lazy = CP.lazy_losses
    CP.lazy_losses = True
    try:
        static = [CP.copy(x) for x in batch(0)]
        v = CP.copy(v0)
        step(static, v)                                          # once eagerly, snapshot off
        arena = LossArena(8, ring_len=ring_len).arm()            # before the capture, as the trainer does
        arena.ring.t.fill_(float('nan'))
        CP.loss_arena = arena
        rt.set_loss_snapshot(arena)
        try:
            with rt.capture(torch.cuda.MemPool()) as graph:
                scalars = step(static, v)
        finally:
            CP.loss_arena = None
            rt.set_loss_snapshot(None)
        index = [arena.index_of(s.t) for s in scalars]
        assert index == [0, 1, 2, 3] and arena.used == 4
        assert int(CP.asnumpy(arena.counter)[0]) == 0 and arena.rows == 0      # capturing runs nothing
        named, refs = [], []
        for j in range(replays):
            b = batch(j)
            for dev, host in zip(static, b):
                dev.set(host)
            graph.replay()
            named.append(arena.next_row())
            refs.append(oracle(b))
        rt.synchronize()
        assert int(CP.asnumpy(arena.counter)[0]) == replays == arena.rows
        cap = arena.array.shape[0]
        ring = CP.asnumpy(arena.ring).reshape(ring_len, cap)
        names = ('softmax CE', 'sigmoid CE', 'Dice', 'regularisation')
        for j, row in enumerate(named):
            assert row.ptr == arena.ring.ptr + (j % ring_len) * cap * 8, f'replay {j}: next_row() named another row'
        for r in range(ring_len):
            j = max(k for k in range(replays) if k % ring_len == r)
            same_bits(CP.asnumpy(named[j]), ring[r], f'row {r} through the view next_row() returned at replay {j}')
            for i, name in zip(index, names):
                loss_close(ring[r, i], refs[j][i], TOL[dtype], f'row {r} = replay {j}: {name}')
                # ... and of no other replay: the four losses of the replays mapped to this row earlier are elsewhere
                for other in range(replays):
                    if other != j:
                        assert abs(ring[r, i] - refs[other][i]) > 100 * TOL[dtype] * max(1.0, abs(refs[other][i])), \
                            f'row {r}: {name} cannot tell replay {j} from {other}'
    finally:
        CP.lazy_losses = lazy
        CP.loss_arena = None


# ---- d. LossArena and the trainer past one lap -------------------------------------------------------------------------------
def flat_losses(losses):
    return list(losses['output_losses']) + [losses['regularization_loss']]


@pytest.mark.gpu
@pytest.mark.parametrize('ring_len', [4, None], ids=['ring4', 'default'])
def test_trainer_past_one_lap(ring_len):
    """ring_len + 6 captured steps over three rotating batches, steps 2 and 3 with the Line net eager
    (set_eager_nets: its tails then run with the snapshot off and advance neither count), all losses kept and read only
    after join().  Truth: the same run read right after every step.  A loss is stale once ring_len further ring rows of
    ITS net have been handed out; with the eager steps this early that is every ring-backed loss older than ring_len
    steps, and none of the last ring_len.  The eager steps' own losses live in slots of their own and read right however
    late.  (trainer.capture() ends with the first replay, which is row 0 of every ring.)"""
    from univer_ocr_amd.hip import HipError
    from univer_ocr_amd.my_model.synthetic import make_page_batch
    from univer_ocr_amd.my_model.trainer import PageTrainer
    from univer_ocr_amd.nn import CP
    CP.use_gpu(0)
    CP.set_dtype('float32')
    extra = {} if ring_len is None else {'snapshot_ring_len': ring_len}
    ring_len = 64 if ring_len is None else ring_len
    steps, eager_at = ring_len + 6, (2, 3)
    batches = [make_page_batch(2, 32, 64, 16, seed=s) for s in (11, 12, 13)]
    lazy = CP.lazy_losses
    CP.lazy_losses = True
    try:
        runs = []
        for late in (False, True):
            trainer = PageTrainer(2, 32, 64, 16, optimizer='sgd', lr=0.01, seed=4, graphs=True, pipelined=True, **extra)
            assert trainer.snapshot_ring_len == ring_len
            trainer.capture(trainer.make_context(batches[0]))
            kept = []
            for i in range(steps):
                if i == eager_at[0]:
                    trainer.set_eager_nets(('Line',))
                elif i == eager_at[-1] + 1:
                    trainer.set_eager_nets(())
                losses = trainer.step(trainer.make_context(batches[i % 3]))
                if late:
                    kept.append({name: flat_losses(l) for name, l in losses.items()})
                else:
                    kept.append({name: [float(x) for x in flat_losses(l)] for name, l in losses.items()})
            trainer.join()
            runs.append((trainer, kept))
        truth, (trainer, kept) = runs[0][1], runs[1]
        assert len({tuple(step['Line']) for step in truth}) == steps          # every step has losses of its own
        rings = {name: entry.arena.ring is not None for name, entry in trainer._captured.items()}
        assert rings['Line'] and set(rings) == set(truth[0])
        stale = fresh = 0
        for name in rings:
            backed = [rings[name] and not (name == 'Line' and i in eager_at) for i in range(steps)]
            arena = trainer._captured[name].arena
            if rings[name]:
                device = int(CP.asnumpy(arena.counter)[0])
                assert arena.rows == device == 1 + sum(backed), f'{name}: host {arena.rows}, device {device}'
            for i in range(steps):
                later = sum(backed[i + 1:])
                expect_stale = backed[i] and later >= ring_len
                if backed[i]:
                    assert expect_stale == (steps - 1 - i >= ring_len), f'{name}, step {i}: the schedule of this test is off'
                for j, value in enumerate(kept[i][name]):
                    if expect_stale:
                        with pytest.raises(HipError, match='snapshot_ring_len'):
                            float(value)
                        stale += 1
                    else:
                        got = float(value)
                        assert got == truth[i][name][j] or (np.isnan(got) and np.isnan(truth[i][name][j])), \
                            f'{name}, step {i}, loss {j}: read late {got!r}, read at once {truth[i][name][j]!r}'
                        fresh += 1
        assert stale and fresh
    finally:
        CP.lazy_losses = lazy

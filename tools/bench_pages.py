#!/usr/bin/env python3
"""The page generator (uocr_page_layout, uocr_page_render) on the batch the step loop trains on: 32 pages of 256 x 512 in
float32, 14 label channels per pixel.

Device time between two events for the layout alone, the render alone (on the tables of rotating batches) and both
together, 30 repetitions per run after a warm-up, 7 runs, the median run reported with the fastest and the slowest; the
page numbers move on with every repetition, so no batch is made twice in a run.  Beside it:
  host path    what the generator replaces: my_model/synthetic.py: make_page_batch on the host (wall time, one batch) and
               the upload of the same five layers, zeros for the `char` layer that make_page_batch lacks (wall time
               around a device synchronise, median of 5)
  write floor  the bytes of the five outputs at the rate of the row `fill (1 write)` of profiles/r03_membw.txt, read from
               that file by this run (measured in round 3 by tools/bench_membw.py, not by this run)
  step         the training step the data feeds, --step-ms: by default the 0.78 ms per 32 pages that DESIGN.md section 6
               records for round 3 (`bench.py`, 41 k pages/s).  `bench.py` reports the step of the
               machine and queue setting it runs with; pass that figure to compare against it (0.93 ms with four hardware
               queues when this tool was added)

    python tools/bench_pages.py > profiles/page_generator_microbench.txt
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

MEMBW_PROFILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'r03_membw.txt')
RECORDED_STEP_MS = 0.78    # bench.py, 32 pages per step
BATCH, H, W = 32, 256, 512
ROTATE = 4


def recorded_fill_gbs():
    """GB/s of the row `fill (1 write)` of profiles/r03_membw.txt"""
    with open(MEMBW_PROFILE) as f:
        row = next(line for line in f if line.startswith('fill (1 write)'))
    return float(row.split()[-2])


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--step-ms', type=float, default=RECORDED_STEP_MS)
    parser.add_argument('--reps', type=int, default=30)
    parser.add_argument('--runs', type=int, default=7)
    args = parser.parse_args()
    from univer_ocr_amd.my_model.pages import GlyphAtlas
    from univer_ocr_amd.my_model.synthetic import make_page_batch
    from univer_ocr_amd.nn import CP, ops
    CP.use_gpu(0)
    CP.set_dtype('float32')
    rt = CP.runtime()
    ev = [ctypes.c_void_p() for _ in range(2)]
    for e in ev:
        assert rt.lib.uocr_event_create(ctypes.byref(e)) == 0
    atlas = GlyphAtlas.shared()
    device, lut = atlas.device(), atlas.lut(np.float32)
    a = device

    tables = [ops.page_layout(device, 1234, BATCH * j, BATCH, H, W) for j in range(ROTATE)]
    outs = [ops.page_render(device, tables[j], H, W, lut) for j in range(ROTATE)]
    order = ('paragraphs', 'lines', 'glyphs', 'counts')
    layers = [name for name, _ in ops.PAGE_LAYERS]

    def layout(i, into=None):
        t = tables[i % ROTATE] if into is None else into
        rt.call('uocr_page_layout', 1234, BATCH * (ROTATE + i), BATCH, H, W, a['metrics'].shape[0], a['metrics'].ptr, a['adv'].ptr,
                *(t[name].ptr for name in order))

    def render(i, of=None):
        t, out = tables[i % ROTATE] if of is None else of, outs[i % ROTATE]
        rt.call('uocr_page_render', 0, BATCH, H, W, *(t[name].ptr for name in order), a['metrics'].shape[0], a['metrics'].ptr,
                a['adv'].ptr, a['offset'].ptr, a['cells'].ptr, a['cells'].shape[0], lut.ptr, *(out[name].ptr for name in layers))

    scratch = ops.page_layout(device, 1234, 0, BATCH, H, W)

    def both(i):
        layout(i, scratch)
        render(i, scratch)

    def timed(fn):
        """microseconds per repetition: the median run, the fastest, the slowest"""
        for i in range(5):
            fn(i)
        runs = []
        for run in range(args.runs):
            rt.synchronize()
            rt.call('uocr_event_record', ev[0])
            for i in range(args.reps):
                fn(run * args.reps + i)
            rt.call('uocr_event_record', ev[1])
            ms = ctypes.c_float()
            assert rt.lib.uocr_event_elapsed_ms_sync(ev[0], ev[1], ctypes.byref(ms)) == 0
            runs.append(ms.value * 1e3 / args.reps)
        return statistics.median(runs), min(runs), max(runs)

    out_bytes = BATCH * H * W * sum(c for _, c in ops.PAGE_LAYERS) * 4
    fill_gbs = recorded_fill_gbs()
    floor_us = out_bytes / fill_gbs / 1e3
    print(f'page generator, {BATCH} pages of {H} x {W} float32 per call ({out_bytes / 1e6:.1f} MB of layers), on {rt.device_info()["name"]}')
    print(f'{args.runs} runs of {args.reps} calls between two events: median run (fastest .. slowest), measured by this run')
    render_us = both_us = None
    for name, fn in (('layout', lambda i: layout(i)), ('render', lambda i: render(i)), ('layout + render', both)):
        mid, low, high = timed(fn)
        if name == 'render':
            render_us = mid
        if name == 'layout + render':
            both_us = mid
        print(f'{name:16s} {mid:8.1f} us ({low:.1f} .. {high:.1f})  {BATCH / mid * 1e6 / 1e3:9.1f} k pages/s')
    counts = np.concatenate([t['counts'].numpy() for t in tables])
    print(f'the pages hold {counts[:, 0].mean():.1f} paragraphs, {counts[:, 1].mean():.1f} lines and {counts[:, 2].mean():.0f} glyphs on average')
    print(f'write floor: {out_bytes / 1e6:.1f} MB at {fill_gbs:.0f} GB/s (the fill row of profiles/r03_membw.txt, recorded in round 3) = {floor_us:.1f} us; '
          f'render / floor = {render_us / floor_us:.1f}x, {out_bytes / render_us / 1e3:.0f} GB/s written')
    source = 'recorded in DESIGN.md section 6 for round 3' if args.step_ms == RECORDED_STEP_MS else 'given with --step-ms'
    print(f'training step the data feeds: {args.step_ms * 1e3:.0f} us per {BATCH} pages ({source}, not measured by this run); '
          f'render / step = {render_us / (args.step_ms * 1e3):.2f}, layout + render / step = {both_us / (args.step_ms * 1e3):.2f}')

    t0 = time.perf_counter()
    host = make_page_batch(BATCH, H, W)
    host_ms = (time.perf_counter() - t0) * 1e3
    host = {'image': host['image'], 'monochrome': host['monochrome'], 'paragraph': host['paragraph'], 'line': host['line'],
            'char': np.zeros((BATCH, H, W, 9))}
    host = {tag: np.ascontiguousarray(v, np.float32) for tag, v in host.items()}
    uploads = []
    for _ in range(5):
        rt.synchronize()
        t0 = time.perf_counter()
        kept = [CP.copy(v, np.float32) for v in host.values()]
        rt.synchronize()
        uploads.append((time.perf_counter() - t0) * 1e3)
        del kept
    upload_ms = statistics.median(uploads)
    print(f'host path it replaces: make_page_batch {host_ms:.0f} ms (one batch, wall) + upload of the five layers '
          f'{upload_ms:.1f} ms (median of 5, wall, pageable memory) = {host_ms + upload_ms:.0f} ms per batch, '
          f'{(host_ms + upload_ms) * 1e3 / (render_us + 0.0):.0f}x the render')


if __name__ == '__main__':
    main()

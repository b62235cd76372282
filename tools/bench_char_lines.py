#!/usr/bin/env python3
"""The Char net over the lines of a page: ONE pass per page on all lines laid side by side (my_model/model.py:
PackedLinesComponent -- one uocr_pack_lines call, one forward with the gaps set back to zero after every conv + LeakyReLU,
the predictions views of the strip's output) against one pass per line (ModelComponent, the default of
make_predict_system and the reference's form).

Two pages: (a) the three lines of fixture (b) of tests/golden/pred_to_text.npz (32 x 24, 40 and 17) and (b) eight
paragraphs of six lines, each 32 x 160.  Per page the span from the line crops on the device to `char_pred` filed; neither
form reads anything back, so the wall clock ends in a stream synchronisation; the event time is taken on the stream around
the same span.  The two forms ALTERNATE: a run is --reps repetitions of one form, --runs runs of each, 'line' and 'page'
in turn; printed are the median run and the fastest and slowest, per repetition, and the C calls of one page.  Both forms
run the same model, once as make_predict_system builds it (layer by layer) and once with the graph fusions on; their
predictions must agree to float32 rounding.

    python tools/bench_char_lines.py [--reps 30] [--runs 7] > profiles/char_lines_microbench.txt
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--reps', type=int, default=30)
    parser.add_argument('--runs', type=int, default=7)
    args = parser.parse_args()
    from univer_ocr_amd.my_model.model import CharSelector, PackedLinesComponent, make_char
    from univer_ocr_amd.nn import CP
    from univer_ocr_amd.nn.model_system import ModelComponent
    CP.use_gpu(0)
    CP.set_dtype('float32')
    rt = CP.runtime()
    ev = [ctypes.c_void_p() for _ in range(2)]
    for e in ev:
        assert rt.lib.uocr_event_create(ctypes.byref(e)) == 0

    def run(fn):
        """(event us, wall us) per repetition of one run"""
        rt.synchronize()
        start = time.perf_counter()
        rt.call('uocr_event_record', ev[0])
        for _ in range(args.reps):
            fn()
        rt.call('uocr_event_record', ev[1])
        ms = ctypes.c_float()
        assert rt.lib.uocr_event_elapsed_ms_sync(ev[0], ev[1], ctypes.byref(ms)) == 0
        return ms.value * 1e3 / args.reps, (time.perf_counter() - start) * 1e6 / args.reps

    golden = np.load(os.path.join(ROOT, 'tests', 'golden', 'pred_to_text.npz'))
    rng = np.random.default_rng(160)
    pages = (('fixture, 2 + 1 lines of 32 x 24, 40, 17', [[golden['system/mono0_0'], golden['system/mono0_1']], [golden['system/mono1_0']]]),
             ('8 paragraphs of 6 lines of 32 x 160', [[rng.random((1, 32, 160, 1)) for _ in range(6)] for _ in range(8)]))
    print(f'Char net per page, one pass on all lines side by side against one pass per line, float32, on '
          f'{rt.device_info()["name"]}: {args.runs} alternating runs of {args.reps} repetitions each, us per repetition as '
          f'median (fastest .. slowest) of the runs')
    for fused in (False, True):
        model = make_char((1, 32, 64, 1))
        if fused:
            model.enable_fusion()
        selector = lambda: CharSelector('cropped_2_monochrome', None, 'char_pred')
        components = {'line': ModelComponent('Char', model, selector(), delist_result=True),
                      'page': PackedLinesComponent('Char', model, selector(), delist_result=True)}
        print(f'-- the model {"with the graph fusions on (enable_fusion)" if fused else "layer by layer, as make_predict_system builds it"}')
        for name, host_lines in pages:
            crops = [[CP.copy(x) for x in paragraph] for paragraph in host_lines]
            filed, calls = {}, {}

            def page_pass(form):
                context = {'cropped_2_monochrome': crops, 'prediction': {}}
                components[form].predict(context)
                filed[form] = context['char_pred']
            forms = [(form, (lambda form=form: page_pass(form))) for form in components]
            for form, fn in forms:                                      # warm-up, and the C calls of one page
                for _ in range(3):
                    before = rt.launches
                    fn()
                    calls[form] = rt.launches - before
            worst = 0.0
            for per_line, per_page in zip(filed['line'], filed['page']):
                for a, b in zip(per_line, per_page):
                    a, b = CP.asnumpy(a), CP.asnumpy(b)
                    assert a.shape == b.shape
                    worst = max(worst, float(np.max(np.abs(a - b)) / np.max(np.abs(a))))
            assert worst < 5e-4, worst
            times = {form: [] for form, _ in forms}
            for _ in range(args.runs):
                for form, fn in forms:
                    times[form].append(run(fn))
            lines = sum(len(p) for p in crops)
            columns = sum(x.shape[2] for p in crops for x in p) + 4 * (lines - 1)
            print(f'{name}: {lines} lines, a strip of {columns} columns; the two forms differ by {worst:.1e} of the largest output')
            for form, _ in forms:
                event, wall = ([t[i] for t in times[form]] for i in (0, 1))
                what = f'{calls[form]:4d} C calls, {lines} passes' if form == 'line' else \
                    f'{calls[form]:4d} C calls, 1 pass, {rt.last_pack_lines()[2]} kernel per pack / zero-gaps call'
                print(f'  {form:5s} {what} | events {statistics.median(event):8.1f} ({min(event):.1f} .. {max(event):.1f}) us | '
                      f'wall clock {statistics.median(wall):8.1f} ({min(wall):.1f} .. {max(wall):.1f}) us')
            by = {form: [statistics.median(t[i] for t in times[form]) for i in (0, 1)] for form, _ in forms}
            print(f'  line / page: {by["line"][0] / by["page"][0]:.2f} by the events, {by["line"][1] / by["page"][1]:.2f} by the wall clock')


if __name__ == '__main__':
    main()

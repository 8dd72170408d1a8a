"""Dev tool: what the no-repeat-n-gram ban costs inside the beam-search and sampling updates (mxvl_beam_step, mxvl_sample_step).

    python tools/ngram_bench.py

One process, one box, one binary: every shape is timed with no_repeat_ngram_size = 0 and = 2 / 3, the arms interleaved in blocks of 100
calls (HIP events around every call, host call included, median of 300 after 20 warm-ups).  The state is reset every 100 calls
(max_new 128, min_new 128: the search never stops), so the history the ban walks grows from 0 to 99 tokens as in a real report.  The
logits repeat call after call, so the histories repeat tokens and the ban fires.  One JSON line per shape."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from medical_image_analysis_amd.report_decoder import _BeamState, _SampleState  # noqa: E402

dev = "cuda:0"
ARMS = (0, 2, 3)


def _time_arms(states, logits, blocks=3, warm=20):
    """{n: median us per call}; arm after arm in blocks of 100 calls, each block from a reset state."""
    times = {n: [] for n in states}
    for n, st in states.items():
        st.reset()
        for _ in range(warm):
            st._advance_hip(logits)
    for _ in range(blocks):
        for n, st in states.items():
            st.reset()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(100)]
            for a, b in ev:
                a.record()
                st._advance_hip(logits)
                b.record()
            torch.cuda.synchronize()
            times[n] += [a.elapsed_time(b) * 1e3 for a, b in ev]
    return {n: round(statistics.median(v), 2) for n, v in times.items()}


def main():
    for V in (32000, 151936):
        for B, nb in ((1, 3), (6, 3), (16, 5)):
            logits = torch.randn(B * nb, V, device=dev) * 4
            for split in (True, False):
                states = {n: _BeamState(B, nb, V, 128, 0, [2], 128, 2.0, 2.0, False, dev, n) for n in ARMS}
                for st in states.values():
                    st.split_vocab = split
                    assert st._hip_supported(logits)
                us = _time_arms(states, logits)
                print(json.dumps(dict(bench="beam_update_ngram", vocab=V, batch=B, beams=nb, split_vocab=split, us_by_n=us,
                                      n2_over_n0=round(us[2] / us[0], 3), n3_over_n0=round(us[3] / us[0], 3))), flush=True)
        for rows in (1, 16, 80):
            logits = torch.randn(rows, V, device=dev) * 4
            states = {n: _SampleState(rows, V, 128, 0, [2], 128, 2.0, 0.8, 50, 0.9, dev, n) for n in ARMS}
            for st in states.values():
                st.seed.fill_(1234)
                assert st._hip_supported(logits)
            us = _time_arms(states, logits)
            print(json.dumps(dict(bench="sample_update_ngram", vocab=V, rows=rows, filters="top_k50+top_p0.9", us_by_n=us,
                                  n2_over_n0=round(us[2] / us[0], 3), n3_over_n0=round(us[3] / us[0], 3))), flush=True)


if __name__ == "__main__":
    main()

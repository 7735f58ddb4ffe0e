"""The launch record of the front end: which library calls a burst makes, with how many frames each and on which stream,
per configuration — the grouping of the frames into launches (super_resolution.front_groups), the per-frame paths
(config.hip.batch: false, timers, grey methods and alignments without a list form, given flows), the graph capture of
host-resident bursts, the alignment-only and the sub-image pipelines.

The expected records (tests/golden/front_end_calls.json) are fixtures: they were written by this module's `--write` main
(with the repository root and the package folder on PYTHONPATH) at the commit BEFORE the four copies of the front end became one
chain, and only a change that means to alter the work on the GPU regenerates them."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from helpers import base_config, recorded_calls

pytestmark = pytest.mark.gpu

import handheld_super_resolution as hsr  # noqa: E402
from handheld_super_resolution import synthetic as synth  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "front_end_calls.json")
DEV = "cuda"
H, W, TS = 384, 512, 16
HIP = {"chunk": 3, "streams": 2}


def _config(hip=None, **kw):
    cfg = base_config(ts=TS, scale=2, metrics=("L1", "L2", "L2", "L2"), **kw)
    cfg.block_matching.tuning.factors = [1, 2, 2, 2]
    cfg.hip = dict(HIP, **(hip or {}))
    return cfg


def _burst(n_comp=5):
    return synth.make_burst(H, W, n_comp + 1, seed=52, max_shift=2.0)[:2]


def _flows(n, given):
    rng = np.random.default_rng(7)
    return [rng.uniform(-1.5, 1.5, (H // TS, W // TS, 2)).astype(np.float32) if i in given else None for i in range(n)]


def _main(cfg, n_comp=5):
    ref, comp = _burst(n_comp)
    hsr.main(torch.as_tensor(ref, device=DEV), torch.as_tensor(comp, device=DEV), cfg)


def _robustness_off():
    cfg = _config()
    cfg.robustness.enabled = False
    cfg.robustness.save_mask = False
    _main(cfg)


def _bilinear():
    cfg = _config()
    cfg.block_matching.tuning.flow_upscale_mode = "bilinear"
    _main(cfg)


def _host_replay():
    ref, comp = _burst(7)
    ref_h, comp_h = torch.from_numpy(ref).pin_memory(), [torch.from_numpy(comp[i]).pin_memory() for i in range(7)]
    cfg = _config({"chunk": 4})
    for _ in range(3):  # eager, capture (chunks of 4, 1, 1, 1 frames), replay
        hsr.main(ref_h, comp_h, cfg)
    from handheld_super_resolution import super_resolution as sr

    runner = [r for c, _, r in sr._main_runners if c is cfg][0]
    assert not runner.disabled and [len(c) for c in next(iter(runner.states.values())).chunks] == [4, 1, 1, 1]


def _align_frames():
    ref, comp = _burst(3)
    pipe = hsr.BurstPipeline(_config()).init_ref(torch.as_tensor(ref, device=DEV), robustness=False)
    pipe.align_frames([torch.as_tensor(comp[i], device=DEV) for i in range(3)])


def _sub_image():
    """The sub-image pipeline of distributed.SlabWork: the reference-frame state of the raw rows [S0, S1), the frames' row
    slabs and the matching tile rows (views) of their full flow fields."""
    ref, comp = _burst()
    ref, comp = torch.as_tensor(ref, device=DEV), torch.as_tensor(comp, device=DEV)
    S0, S1 = 128, 256
    t0, t1, ny = S0 // TS, S1 // TS, H // TS
    flows = [torch.as_tensor(f, device=DEV) for f in _flows(5, range(5))]
    sub = hsr.BurstPipeline(_config())
    sub.init_ref(ref[S0:S1], alignment=False)
    sub.flow_rows = (t0, ny - t1)
    sub.process_frames([comp[i][S0:S1] for i in range(5)], None, fuse_local_min=True, flows=[f[t0:t1] for f in flows])


CASES = {
    "default": lambda: _main(_config()),
    "batch_off": lambda: _main(_config({"batch": False})),
    "mode_grey": lambda: _main(_config(mode="grey")),
    "robustness_off": _robustness_off,
    "flows_all": lambda: _main(_config({"inject_flows": _flows(5, range(5))})),
    "flows_some": lambda: _main(_config({"inject_flows": _flows(5, (1, 3))})),
    "verbose_2": lambda: _main(_config(verbose=2)),
    "flow_upscale_bilinear": _bilinear,
    "grey_fft_torch": lambda: _main(_config(grey_method="FFT_torch")),
    "host_burst_replay": _host_replay,
    "align_frames": _align_frames,
    "sub_image": _sub_image,
}


def _record(case):
    with recorded_calls() as records:
        CASES[case]()
        torch.cuda.synchronize()
    return records


@pytest.mark.parametrize("case", list(CASES))
def test_front_end_calls(case):
    with open(GOLDEN) as f:
        want = json.load(f)[case]
    got = _record(case)
    assert got == want, next((i, g, w) for i, (g, w) in enumerate(zip(got + [None], want + [None])) if g != w)


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: test_front_end_calls.py --write   (rewrites the fixture from the code as it is: see the docstring)")
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f'"{c}": {json.dumps(_record(c), separators=(",", ":"))}' for c in CASES) + "\n}\n")

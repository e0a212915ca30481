"""Seeded slices of the two randomised sweeps of the training step, collected by pytest.

tests/stress_step.py (fused step vs the oracle over random shapes, `big` = the item-partitioned forward's range) and
tools/stress_pipeline.py (in-launch pipeline vs side-stream prefetch, bit for bit) found real bugs but run only by hand
and by the clock.  Here: fixed seeds and a fixed number of cases per seed, so two runs execute the same cases.  The
seeds are chosen so that the library refuses none of these cases up front and every pipeline case really pipelines
(no sampled softmax, no D = 768: those have no pipeline); a case that comes back refused or un-pipelined fails, so
nothing is silently left out if the sweeps' draws change."""
import os
import sys

import numpy as np
import pytest

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)

pytestmark = pytest.mark.gpu

STEP_SEEDS, STEP_CASES = (2, 4, 7), 6            # every shape class: D 6 .. 2048, batches 1 .. 4500, all three losses
BIG_SEEDS, BIG_CASES = (7, 11, 12), 4            # D 256 .. 2048, batches >= 2048, item tables of 5 .. 40 MB
PIPE_SEEDS, PIPE_CASES, PIPE_DIMS = (7, 9, 12), 4, (256, 512, 1024)


@pytest.mark.parametrize('big,seed', [(False, s) for s in STEP_SEEDS] + [(True, s) for s in BIG_SEEDS],
                         ids=[f'plain-{s}' for s in STEP_SEEDS] + [f'big-{s}' for s in BIG_SEEDS])
def test_stress_step_slice(oracle, big, seed):
    import stress_step
    rng = np.random.RandomState(seed)
    for k in range(BIG_CASES if big else STEP_CASES):
        ok, desc = stress_step.one_case(rng, big)
        assert ok is not None, f'case {k} of seed {seed} was refused up front: {desc}'
        assert ok is True, f'case {k} of seed {seed} is off the oracle: {desc}'


@pytest.mark.parametrize('seed', PIPE_SEEDS)
def test_stress_pipeline_slice(seed):
    import stress_pipeline
    from hassaku_amd import hip_ops
    lib = hip_ops._lib.load()
    rng = np.random.RandomState(seed)
    try:
        for k in range(PIPE_CASES):
            ok, desc = stress_pipeline.one_case(rng, lib, PIPE_DIMS)
            assert ok and not desc['diff'], f'case {k} of seed {seed}: pipelined and side-stream runs differ: {desc}'
            assert desc['pipelined_steps'] > 0, f'case {k} of seed {seed} did not pipeline: {desc}'
    finally:
        lib.hsk_bprmf_set_pipeline(1)

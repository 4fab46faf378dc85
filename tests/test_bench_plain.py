"""bench.py's plain run on CPU with the mock device store: it prints the
headline result line without the --full legs, --steps sets the number of
timed steps, and --dump-outputs writes float arrays that do not depend on how
many spin-up steps happened to fit before the warmup."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from test_bench_multiproc import MockStore

HEADLINE_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype",
                 "ms_per_step", "steps", "warmup", "n_gpus"}
FULL_ONLY_KEYS = {"cross_shard_range", "compact_sweep", "watch_events_per_sec",
                  "watch_stats", "ops_per_sec_with_d2h",
                  "ops_per_sec_with_d2h_keys_only", "d2h_detail",
                  "pcie_d2h_GBps", "box", "cpu_baseline",
                  "cpu_baseline_full_config"}
STEPS = 5
SHAPE = ["--steps", str(STEPS), "--warmup", "2", "--nns", "16", "--per-ns",
         "40", "--extra-revs", "50", "--watchers", "4", "--watch-events", "30"]


class CountingStore(MockStore):
    def __init__(self, **kw):
        super().__init__(**kw)
        self.step_calls = []  # ntx of every kb_bench_step call

    def f_bench_step(self, h, qblob, nq, tblob, ntx, *rest):
        self.step_calls.append(ntx.value)
        return super().f_bench_step(h, qblob, nq, tblob, ntx, *rest)


def _run(extra, outdir):
    """One bench.main() over a fresh mock store; returns (line, store)."""
    import contextlib
    import io

    import kubebrain_amd
    stores = []

    def opener(**kw):
        stores.append(CountingStore(**kw))
        return stores[-1]

    kubebrain_amd.open_store = opener
    import bench
    sys.argv = ["bench.py"] + SHAPE + extra
    cap = io.StringIO()
    with contextlib.redirect_stdout(cap):
        bench.main()
    lines = cap.getvalue().strip().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0]), stores[0]


def _worker(outdir):
    os.environ.update({"RANK": "0", "WORLD_SIZE": "1"})
    d1, d2 = os.path.join(outdir, "a"), os.path.join(outdir, "b")
    line, st = _run(["--spin-up", "0", "--dump-outputs", d1], outdir)
    assert HEADLINE_KEYS <= set(line), sorted(line)
    assert not (FULL_ONLY_KEYS & set(line)), sorted(FULL_ONLY_KEYS & set(line))
    assert line["steps"] == STEPS and line["ms_per_step"] > 0
    # no spin-up: exactly warmup + steps calls, every one with its txn batch
    assert st.step_calls == [100] * (2 + STEPS), st.step_calls
    # a spin-up of unknown length before the same warmup + steps
    line2, st2 = _run(["--spin-up", "0.05", "--dump-outputs", d2], outdir)
    spin = len(st2.step_calls) - (2 + STEPS)
    assert spin > 0 and st2.step_calls[:spin] == [0] * spin  # range-only
    assert st2.step_calls[spin:] == [100] * (2 + STEPS)
    names = sorted(os.listdir(d1))
    assert names == sorted(os.listdir(d2)) and len(names) >= 5
    total = 0
    for n in names:
        a, b = np.load(os.path.join(d1, n)), np.load(os.path.join(d2, n))
        assert a.dtype in (np.float32, np.float64), (n, a.dtype)
        assert a.shape == b.shape and np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(os.path.join(d1, "step_range_totals.npy")).shape == (STEPS,)
    assert np.load(os.path.join(d1, "txn_revisions.npy")).shape == (100,)
    # --full adds the other legs' keys to the same headline
    line3, _ = _run(["--spin-up", "0", "--full", "--no-cpu-baseline"], outdir)
    assert HEADLINE_KEYS <= set(line3)
    assert FULL_ONLY_KEYS <= set(line3), sorted(FULL_ONLY_KEYS - set(line3))
    assert line3["watch_events_per_sec"] is not None


def test_value_stream_matches_per_byte_draws():
    """The loader draws value bytes as full-range uint32 words; that must be
    the byte stream (and leave the generator in the state) of one uint8 draw
    per byte, which is how the benchmark's inputs are defined."""
    for n in (4, 512, 3 * 512 * 1024):
        a, b = np.random.default_rng(0x6B62), np.random.default_rng(0x6B62)
        x = a.integers(0, 256, size=n, dtype=np.uint8)
        y = b.integers(0, 1 << 32, size=n // 4, dtype=np.uint32).view(np.uint8)
        assert np.array_equal(x, y)
        assert np.array_equal(a.zipf(1.1, size=8), b.zipf(1.1, size=8))
        assert np.array_equal(a.integers(0, 256, size=16, dtype=np.uint8),
                              b.integers(0, 256, size=16, dtype=np.uint8))


def test_bench_plain_full_and_dump(tmp_path):
    import torch.multiprocessing as mp

    p = mp.get_context("spawn").Process(target=_worker, args=(str(tmp_path),))
    p.start()
    p.join(240)
    assert p.exitcode == 0, p.exitcode

"""What kernel_time() reports after sample_kernel(every), per sampling site.

Each path of a queue run, a window run and a what-if step brackets one of its
launches with a pair of events when sampling is on; kernel_time() averages the
pairs of the last run.  bench.py --full and bench_whatif.py build their roofline
on that figure.  Per site, on the smallest cluster that reaches it: the number
of samples (read off the site's gating condition), a positive average, and the
path counters that show the intended path ran.

The node-sharded sites (window_split, the X1..X4 chains) need one process
per rank, as tests/test_distributed.py starts them; they are not covered here.
"""
import pytest

from ksg import Scheduler, generator as g

BATCH = 32  # pods per window (KSG_BATCH)


def _ceil(a, b):
    return (a + b - 1) // b


def _run(doc, every, per_pod=None, whatif=False):
    s = Scheduler(doc["profile"])
    s.load_cluster(doc)
    if per_pod is not None:
        s.set_path(per_pod)
    s.sample_kernel(every)
    if whatif:
        s.whatif(0, s.queue_len)
    else:
        s.schedule()
    ms, n = s.kernel_time()
    print(f"samples={n} avg_ms={ms:.5f} paths={s.path_counts()} runs={s.run_counts()} "
          f"window_runs={s.window_runs()} class_chunks={s.whatif_class_chunks()}")
    assert ms > 0
    return s, n


@pytest.mark.gpu
@pytest.mark.parametrize("every", [1, 7])
def test_static_chain_samples_every_nth_pod(every):
    """cfg3 per pod (k_static + k_fs_static): the k_fs_static of each pod j with
    j % every == 0; the static chain counts no table- or scanning-chain pod."""
    doc = g.generate(3, n_nodes=200, n_pods=40)
    s, n = _run(doc, every, per_pod=True)
    assert not s.batch_path
    assert n == _ceil(40, every)
    assert s.path_counts() == (0, 0) and s.window_runs() == 0


CFG4 = dict(n_nodes=200, n_existing=600, n_pods=40, n_zones=4)


@pytest.mark.gpu
def test_persistent_segments_sample_each_segment():
    """cfg4: every pod is eligible and of one size class, so the queue is one
    persistent segment (k_chain_run) and one sample, whatever `every` is."""
    s, n = _run(g.generate(4, **CFG4), 3)
    assert s.path_counts() == (40, 0)
    assert s.run_counts() == (40, 1)
    assert n == 1


@pytest.mark.gpu
@pytest.mark.parametrize("every", [1, 3])
def test_table_chain_samples_every_nth_pod(monkeypatch, every):
    """The same queue on the two-launch table chain (KSG_RUN=0): the k_eval of
    each pod j with j % every == 0."""
    monkeypatch.setenv("KSG_RUN", "0")
    s, n = _run(g.generate(4, **CFG4), every)
    assert s.path_counts() == (40, 0)
    assert s.run_counts() == (0, 0)
    assert n == _ceil(40, every)


@pytest.mark.gpu
@pytest.mark.parametrize("every", [1, 4])
def test_scanning_chain_samples_every_nth_pod(every):
    """Default-profile pods whose spread constraint honours node taints are not
    table-eligible: the scanning chain, the k_filter_score of each pod j with
    j % every == 0."""
    doc = g.generate(1, n_nodes=60, n_pods=10)
    for p in doc["queue"]:
        p["spec"]["topologySpreadConstraints"] = [{
            "maxSkew": 1, "topologyKey": g.ZONE, "whenUnsatisfiable": "ScheduleAnyway",
            "labelSelector": {"matchLabels": {"app": p["metadata"]["labels"]["app"]}}, "nodeTaintsPolicy": "Honor"}]
    s, n = _run(doc, every)
    assert s.path_counts() == (0, 10)
    assert s.run_counts() == (0, 0)
    assert n == _ceil(10, every)


WINDOWS = 96 // BATCH


@pytest.mark.gpu
@pytest.mark.parametrize("every", [1, 5])
def test_persistent_window_loop_is_one_sample(every):
    """cfg2, 96 pods: the three windows run inside one k_window_run launch,
    sampled whatever `every` is."""
    s, n = _run(g.generate(2, n_nodes=300, n_pods=96), every)
    assert s.batch_path
    assert s.window_runs() == 1
    assert n == 1


@pytest.mark.gpu
@pytest.mark.parametrize("every", [1, 5])
def test_per_window_launches_sample_full_launches(monkeypatch, every):
    """KSG_WIN_RUN=0: windows + 1 k_window launches, of which the windows - 1 that
    both evaluate a window and replay the one before are sampled, whatever
    `every` is."""
    monkeypatch.setenv("KSG_WIN_RUN", "0")
    s, n = _run(g.generate(2, n_nodes=300, n_pods=96), every)
    assert s.batch_path
    assert s.window_runs() == 0
    assert n == WINDOWS - 1


@pytest.mark.gpu
@pytest.mark.parametrize("every", [1, 5])
def test_static_window_loop_is_one_sample(every):
    """cfg3, 96 pods: the persistent window loop over static records."""
    s, n = _run(g.generate(3, n_nodes=300, n_pods=96), every)
    assert s.batch_path
    assert s.window_runs() == 1
    assert n == 1


@pytest.mark.gpu
@pytest.mark.parametrize("classes", [True, False], ids=["class-path", "record-path"])
def test_whatif_samples_both_passes_of_first_chunk(monkeypatch, classes):
    """A what-if step: one sample per pass of its first chunk of pods, on the
    class path (k_whatif_cls1/2) and, with KSG_WHATIF_CLASSES=0, the record path."""
    if not classes:
        monkeypatch.setenv("KSG_WHATIF_CLASSES", "0")
    s, n = _run(g.generate(5, n_nodes=300, n_pods=96), 1, whatif=True)
    assert s.whatif_class_chunks() == (1 if classes else 0)
    assert n == 2

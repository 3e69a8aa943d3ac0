"""``mxnet_sparse_linear.py`` through the launcher on CPU ranks (1 scheduler + 1 server + 2 workers, dist_sync, the
payloads over gloo): the loss falls, and because every merge of the store is ordered the final table of a rerun is
the same bit for bit."""
import pytest

from test_jobs_local import _diag, _metrics, conf, run_job  # noqa: F401 - conf is a fixture

pytestmark = pytest.mark.timeout(300)

PARAMS = ("--kvstore dist_sync --device cpu --features 512 --dim 8 --samples 4096 --batch-size 256 --epochs 3 "
          "--lr 0.02")


def _run(conf):  # noqa: F811
    rc, client, _ = run_job(conf, "mxnet_sparse_linear.py",
                            ["tony.application.framework=mxnet", "tony.scheduler.instances=1",
                             "tony.server.instances=1", "tony.worker.instances=2", "tony.ps.instances=0"], PARAMS)
    assert rc == 0, _diag(client)
    return _metrics(client)


def test_sparse_linear_job_learns_and_is_reproducible(conf, tmp_path):  # noqa: F811
    ms = _run(conf)
    for rank in (0, 1):
        loss = [m["loss"] for m in sorted((m for m in ms if m.get("rank") == rank and "epoch" in m),
                                          key=lambda m: m["epoch"])]
        assert len(loss) == 3 and loss[2] < loss[1] < loss[0], loss
        assert all(m["samples_per_s"] > 0 for m in ms if "epoch" in m)
    final = {m["rank"]: m["table_sha256"] for m in ms if m.get("final")}
    assert sorted(final) == [0, 1] and final[0] == final[1]  # both workers pull the same table
    conf.set("tony.amd.staging-dir", str(tmp_path / "staging2"))
    again = {m["rank"]: m["table_sha256"] for m in _run(conf) if m.get("final")}
    assert again == final  # a rerun ends on the same bits


def test_the_job_takes_only_known_devices():
    from tony_amd.jobs import mxnet_sparse_linear

    with pytest.raises(SystemExit) as e:
        mxnet_sparse_linear.main(["--device", "tpu"])
    assert e.value.code == 2  # argparse's usage error, before any role runs

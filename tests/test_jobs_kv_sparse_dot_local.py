"""``mxnet_sparse_linear.py --dot csr`` through the launcher on CPU ranks, the set-up of test_jobs_kv_sparse_local.py:
the step goes through ``kv.dot``; the loss falls, both workers end on one table, a rerun on the same bits."""
import pytest

import test_jobs_kv_sparse_local as base
from test_jobs_local import conf  # noqa: F401 - a fixture

pytestmark = pytest.mark.timeout(300)


def test_sparse_linear_job_with_csr_dot_learns_and_is_reproducible(conf, tmp_path, monkeypatch):  # noqa: F811
    monkeypatch.setattr(base, "PARAMS", base.PARAMS + " --dot csr")
    ms = base._run(conf)
    assert all(m["dot"] == "csr" for m in ms if "epoch" in m or m.get("final"))
    for rank in (0, 1):
        loss = [m["loss"] for m in sorted((m for m in ms if m.get("rank") == rank and "epoch" in m),
                                          key=lambda m: m["epoch"])]
        assert len(loss) == 3 and loss[2] < loss[1] < loss[0], loss
    final = {m["rank"]: m["table_sha256"] for m in ms if m.get("final")}
    assert sorted(final) == [0, 1] and final[0] == final[1]
    conf.set("tony.amd.staging-dir", str(tmp_path / "staging2"))
    assert {m["rank"]: m["table_sha256"] for m in base._run(conf) if m.get("final")} == final

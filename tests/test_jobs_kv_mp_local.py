"""``mxnet_linreg.py --key-dtype bf16 --multi-precision`` through the launcher on CPU ranks (1 scheduler + 1 server + 2
workers, dist_sync, the payloads over gloo) converges like the fp32 job of tests/test_jobs_local.py, and the default
invocation prints what it printed."""
import json
import re

import pytest

from test_jobs_local import _diag, _metrics, conf, run_job  # noqa: F401 - conf is a fixture

pytestmark = pytest.mark.timeout(300)


def test_linreg_job_on_multi_precision_bf16_keys(conf):  # noqa: F811
    rc, client, _ = run_job(conf, "mxnet_linreg.py",
                            ["tony.application.framework=mxnet", "tony.scheduler.instances=1",
                             "tony.server.instances=1", "tony.worker.instances=2", "tony.ps.instances=0"],
                            "--kvstore dist_sync --rows 8192 --epochs 3 --lr 0.5 --key-dtype bf16 --multi-precision")
    assert rc == 0, _diag(client)
    ms = _metrics(client)
    assert ms and all(m["key_dtype"] == "bf16" for m in ms)
    assert all(m["mse"] < 0.05 for m in ms if m["epoch"] == 2)


def test_the_default_invocation_prints_what_it_printed(monkeypatch, capfd):
    from tony_amd.jobs import mxnet_linreg

    monkeypatch.delenv("DMLC_ROLE", raising=False)
    assert mxnet_linreg.main(["--kvstore", "local", "--rows", "4096", "--epochs", "2", "--lr", "0.5"]) == 0
    out, err = capfd.readouterr()
    lines = [ln for ln in (out + err).splitlines() if ln.strip()]
    metrics = [json.loads(ln[len("TONY_METRIC "):]) for ln in lines if ln.startswith("TONY_METRIC ")]
    assert [sorted(m) for m in metrics] == [["epoch", "mse", "rank"]] * 2
    rest = [ln for ln in lines if not ln.startswith("TONY_METRIC ")]
    assert len(rest) == 1 and re.search(r"worker 0/1: w=\d\.\d{3} b=\d\.\d{3} mse=\d\.\d{5}$", rest[0]), rest

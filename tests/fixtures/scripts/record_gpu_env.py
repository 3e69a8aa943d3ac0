"""Writes this task's GPU pinning env to $RECORD_DIR/<job>_<index>.txt (ps / worker placement tests).

A ps task is untracked: the coordinator stops it as soon as every worker has finished, which on a busy host can
be before its script has run.  So a worker leaves only once every task of the cluster spec has written its
record (a bounded wait that normally ends within milliseconds), and each record appears atomically."""
import json
import os
import time

d = os.environ["RECORD_DIR"]
keys = ("TONY_GPU_IDS", "TONY_HIP_ORDINALS", "TONY_VISIBLE_MODE", "HIP_VISIBLE_DEVICES", "TONY_PS_SHARED_GPU",
        "TONY_PS_GPUS")
path = os.path.join(d, f"{os.environ['JOB_NAME']}_{os.environ['TASK_INDEX']}.txt")
with open(path + ".part", "w") as f:
    for k in keys:
        f.write(f"{k}={os.environ.get(k, '')}\n")
os.replace(path + ".part", path)

if os.environ["JOB_NAME"] != "ps":
    spec = json.loads(os.environ.get("CLUSTER_SPEC") or "{}")
    want = [os.path.join(d, f"{job}_{i}.txt") for job, hosts in spec.items() for i in range(len(hosts))]
    deadline = time.monotonic() + 30
    while time.monotonic() < deadline and not all(os.path.exists(w) for w in want):
        time.sleep(0.02)

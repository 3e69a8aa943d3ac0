"""The flat optimizers compute, bit for bit, what they computed before the four kinds were folded onto one apply
kernel: tests/golden/optim_bits.json holds the sha256 digests that tools/optim_bits.py printed on an MI355X in a
checkout of the commit before the fold (the tool uses only the public ``Flat*`` API, so the same file ran there).
Every case is element-wise and free of atomics, so equality is exact; the cases and sizes are in the tool's
docstring."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "optim_bits.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def digests(cuda):
    spec = importlib.util.spec_from_file_location("optim_bits", os.path.join(ROOT, "tools", "optim_bits.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool.digests(cuda)  # every case once, shared by the tests below


@pytest.mark.gpu
def test_same_cases_as_golden(digests):
    assert sorted(digests) == sorted(GOLDEN)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(GOLDEN))
def test_bits_match_parent(digests, case):
    assert digests[case] == GOLDEN[case]

"""``tony_topk_count`` (csrc/metrics.hip) against the strictly-greater count on the CPU: the counters must be equal
exactly -- ties that straddle the k boundary, a target at rank k and k+1, non-finite target logits, a row stride
with +inf padding, fewer classes than one wave, and two launches into the same counters."""
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 5


def _cpu_count(logits, targets, k):
    """[hit@1, hit@k, rows]: the target logit is finite and fewer than k classes are strictly greater."""
    x = logits.float().cpu()
    xt = x.gather(1, targets.cpu()[:, None])
    greater = (x > xt).sum(1)
    ok = torch.isfinite(xt[:, 0])
    return [int((ok & (greater < 1)).sum()), int((ok & (greater < k)).sum()), x.shape[0]]


def _constructed(classes, dtype):
    """Rows whose outcome is decided by construction (values exact in bf16); target = class 0 throughout."""
    base = torch.full((8, classes), -1.0)
    rows = []

    def row(target_value, greater, ties):
        r = base[0].clone()
        r[0] = target_value
        r[1:1 + greater] = target_value + 1 if target_value == target_value and abs(target_value) != float("inf") else 1
        r[1 + greater:1 + greater + ties] = target_value
        rows.append(r)

    n = min(classes - 1, K + 1)
    row(2.0, min(K - 1, n), 0)                  # exactly rank k: a hit
    row(2.0, min(K, n), 0)                      # rank k+1: a miss (when there are that many classes)
    row(2.0, min(K - 2, n), min(3, n - min(K - 2, n)))  # a tie straddling the k boundary: a hit
    row(2.0, 0, min(3, n))                      # tied for first: top-1 and top-k
    row(float("-inf"), 0, 0)                    # non-finite targets never hit
    row(float("inf"), 0, 0)
    row(float("nan"), 0, 0)
    r = base[0].clone()                          # a NaN elsewhere is not greater
    r[0], r[1] = 0.5, float("nan")
    rows.append(r)
    return torch.stack(rows).to(dtype), torch.zeros(len(rows), dtype=torch.int64)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,classes,ld", [(5, 1000, 1000), (5, 1001, 1008), (5, 7, 7)])
def test_counters_equal_the_cpu_count(cuda, rows, classes, ld, dtype):
    from tony_amd.ops.metrics import TopK

    g = torch.Generator().manual_seed(classes)
    # bf16 normal logits tie often, which is wanted; targets drawn among the largest so both outcomes occur
    x = torch.randn(rows, classes, generator=g).to(dtype)
    y = x.float().topk(min(classes, 2 * K), dim=1).indices[torch.arange(rows), torch.randint(0, min(classes, 2 * K),
                                                                                            (rows,), generator=g)]
    cx, cy = _constructed(classes, dtype)
    m = TopK(K, cuda)
    want = [0, 0, 0]
    for logits, targets in ((x, y), (cx, cy)):  # two launches accumulate into the same counters
        padded = torch.full((logits.shape[0], ld), float("inf"), dtype=dtype)  # padding columns must be ignored
        padded[:, :classes] = logits
        view = padded.to(cuda)[:, :classes]
        assert view.stride(0) == ld
        m.update(view, targets.to(cuda))
        want = [a + b for a, b in zip(want, _cpu_count(logits, targets, K))]
    assert m.counters.tolist() == want
    top1, topk, seen = m.result()
    assert seen == want[2] and top1 == want[0] / seen and topk == want[1] / seen
    m.reset()
    assert m.counters.tolist() == [0, 0, 0]


def test_constructed_rows_by_hand(cuda):
    """The constructed rows' outcome at 1000 classes, counted by hand: 2 hits@1 (tied for first, and the row with a
    NaN elsewhere), 4 hits@5 (those two, rank 5 exactly, and the straddling tie), 8 rows."""
    from tony_amd.ops.metrics import TopK

    for dtype in (torch.float32, torch.bfloat16):
        cx, cy = _constructed(1000, dtype)
        assert _cpu_count(cx, cy, K) == [2, 4, 8]
        m = TopK(K, cuda)
        m.update(cx.to(cuda), cy.to(cuda))
        assert m.counters.tolist() == [2, 4, 8]

"""engine/merge.py on the GPU: sort_perm, last_row_index and merge_rows on
device tensors equal their CPU results bit for bit, at the sizes where the
kernels change path (a wave is 64 rows)."""

import numpy as np
import pytest
import torch

import _lnn_cases as L
from greptimedb_amd.engine import merge

pytestmark = pytest.mark.gpu


def _rows(lengths):
    """Sorted rows for groups of the given lengths, about half the values NaN
    and the first two rows of the longest group the only non-NaN ones in it."""
    lengths = np.asarray(lengths, dtype=np.int64)
    rng = np.random.default_rng(int(lengths.sum()) + 1)
    se, ts, f = L._from_lengths(lengths, 2, rng, p_nan=0.5)
    if len(lengths) and lengths.max() > 2:
        g = int(lengths.argmax())
        lo = int(lengths[:g].sum())
        f[:, lo + 2: lo + lengths[g]] = L.NAN
        f[:, lo: lo + 2] = [[1.0, 2.0], [3.0, L.NAN]]
    return se, ts, f


CASES = {
    "n0": [],
    "n1": [1],
    # rows 62..64 are one group: it straddles the first wave boundary
    "n65_straddle": [1] * 62 + [3],
    # 64*3 + 1 rows; rows 31..160 are one group of 130, over two boundaries
    "n193_group130": [1] * 31 + [130] + [1] * 32,
}


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_cpu(name):
    se, ts, f = _rows(CASES[name])
    n = len(ts)
    assert n == {"n0": 0, "n1": 1, "n65_straddle": 65,
                 "n193_group130": 193}[name]
    if name == "n65_straddle":
        assert se[62] == se[64] and ts[62] == ts[64]
    dev = torch.device("cuda:0")
    c = [torch.as_tensor(a.copy()) for a in (se, ts, f)]
    g = [t.to(dev) for t in c]

    # the sort, from a fixed shuffle of the rows (ties by shuffled position)
    shuf = torch.as_tensor(np.random.default_rng(n).permutation(n))
    p_cpu = merge.sort_perm(c[0][shuf], c[1][shuf])
    p_gpu = merge.sort_perm(g[0][shuf.to(dev)], g[1][shuf.to(dev)])
    assert p_gpu.is_cuda and p_gpu.dtype == torch.int64
    assert torch.equal(p_gpu.cpu(), p_cpu)
    assert torch.equal(c[0][shuf][p_cpu], c[0])       # and it does sort

    k_cpu = merge.last_row_index(c[0], c[1])
    k_gpu = merge.last_row_index(g[0], g[1])
    assert k_gpu.is_cuda and k_gpu.dtype == torch.int64
    assert torch.equal(k_gpu.cpu(), k_cpu)
    assert k_cpu.numel() == len(CASES[name])

    for mode in ("append", "last_row", "last_non_null"):
        kc, fc = merge.merge_rows(*c, mode)
        kg, fg = merge.merge_rows(*g, mode)
        if mode == "append":
            assert kc is None and kg is None and fg is g[2]
            continue
        assert torch.equal(kg.cpu(), kc)
        L.check(kg.cpu().numpy(), fg.cpu().numpy(), kc.numpy(), fc.numpy())

"""GPU: next_batch_unified(device=cuda) — the seven tensors of a batch staged through one pinned
block and one asynchronous copy — equals the host batches for odd and even sizes and several
negatives per record, with the same Python and NumPy generator states afterwards; the copies keep
their values when the host refills its staging for later batches before the device has read
them (every batch is read only after both epochs have run)."""
import pytest
import torch

from tests import _unified_ref as R
from tests.test_unified_sampler import CASES, _inputs, _run_native, _seed, _states

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_records,batch,batch_kg,n_negs", CASES)
def test_device_batches_equal_host_batches(n_records, batch, batch_kg, n_negs):
    from hypergraph_diffusion_for_recommendation_amd.sampler import next_batch_unified
    dev = torch.device("cuda")
    data, (h, r, t) = _inputs(n_records)
    know = R.knowledge(data.training_data, h, r, t)
    _seed(3)
    want, want_states = _run_native(data, know, batch, batch_kg, n_negs)
    _seed(3)
    got = []
    for _ in range(2):
        ep = []
        for b in next_batch_unified(data, know, batch, batch_kg, n_negs, device=dev):
            assert len(b) == 7
            assert all(x.is_cuda and x.dtype == torch.int64 and x.is_contiguous() for x in b)
            ep.append(b)  # read after the whole run: later batches must not overwrite earlier
        got.append(ep)
    torch.cuda.synchronize()
    assert _states() == want_states
    for e in range(2):
        assert len(got[e]) == len(want[e])
        for b, w in zip(got[e], want[e]):
            assert tuple(x.tolist() for x in b) == w
            assert b[2].numel() == b[0].numel() * n_negs and b[6].numel() == batch_kg

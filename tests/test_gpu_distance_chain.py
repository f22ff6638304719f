"""The use cases behind the distance functions, on device pointers with no host copy in between.

Nearest template: arm_euclidean_distance_f32_batch of one query against 5000 stored templates (bStride 0: the query
is the shared B vector), then arm_min_f32_batch over the 5000 distances names the template the restatement names.

Alignment: a 60 x 70 distance matrix filled on the device, arm_dtw_init_window_q7_batch -> arm_dtw_distance_f32_batch
-> arm_dtw_path_f32_batch; the distance and the path equal the restatement's."""
import numpy as np
import pytest

import distance_ref as dr
from f32_classes import assert_same_words

TEMPLATES, DIM = 5000, 48
Q, T, BAND = 60, 70, 14


@pytest.mark.gpu
def test_nearest_template_on_device(dsp, torch_gpu):
    torch = torch_gpu
    rng = np.random.default_rng(211)
    bank = rng.uniform(-1.0, 1.0, (TEMPLATES, DIM)).astype(np.float32)
    query = (bank[3217] + rng.uniform(-0.05, 0.05, DIM)).astype(np.float32)
    d_bank, d_query = torch.from_numpy(bank).cuda(), torch.from_numpy(query).cuda()
    dist = torch.full((TEMPLATES,), float("nan"), dtype=torch.float32, device="cuda")
    best = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
    index = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    dsp.distance_batch("euclidean", d_bank, d_query, dist)
    dsp.min_batch(dist.view(1, TEMPLATES), best, index)
    torch.cuda.synchronize()
    want = np.array([dr.distance_f32("euclidean", row, query) for row in bank], dtype=np.float32)
    assert_same_words(dist.cpu().numpy(), want, "distances")
    assert int(index[0]) == int(np.argmin(want)) == 3217 and best.cpu().numpy()[0] == want[3217]
    assert d_bank.cpu().numpy().tobytes() == bank.tobytes() and d_query.cpu().numpy().tobytes() == query.tobytes()


@pytest.mark.gpu
def test_dtw_chain_on_device(dsp, torch_gpu):
    torch = torch_gpu
    rng = np.random.default_rng(223)
    query = torch.from_numpy(np.sin(0.21 * np.arange(Q) ** 1.05).astype(np.float32)).cuda()
    templ = torch.from_numpy((np.sin(0.18 * np.arange(T)) + 0.01 * rng.standard_normal(T)).astype(np.float32)).cuda()
    dist = (query[:, None] - templ[None, :]).abs().contiguous().view(1, Q, T)          # filled on the device
    window = torch.full((1, Q, T), 0x5A, dtype=torch.int8, device="cuda")
    cost = torch.full((1, Q, T), float("nan"), dtype=torch.float32, device="cuda")
    result = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
    path = torch.full((1, Q + T, 2), 0x5A5A, dtype=torch.int16, device="cuda")
    length = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    dsp.dtw_init_window_batch(dsp.ARM_DTW_SLANTED_BAND_WINDOW, BAND, window)
    status = dsp.dtw_distance_batch(dist, window, cost, result)
    dsp.dtw_path_batch(cost, path, length)
    torch.cuda.synchronize()
    d = dist.cpu().numpy()[0]
    w = dr.init_window(dr.SLANTED_BAND, BAND, Q, T)
    assert window.cpu().numpy()[0].tobytes() == w.tobytes()
    st, want, wcost = dr.dtw_distance(d, w)
    assert st == 0 and int(status[0]) == 0
    assert_same_words(cost.cpu().numpy()[0], wcost, "cost matrix")
    assert dr.same_word(result.cpu().numpy()[0], want)
    wpath = dr.dtw_path(wcost)
    n = int(length[0])
    assert n == len(wpath) and np.array_equal(path.cpu().numpy()[0, :n], wpath)
    assert tuple(wpath[0]) == (0, 0) and tuple(wpath[-1]) == (Q - 1, T - 1)

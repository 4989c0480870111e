"""Host-side parts of per-shape recorded step lists (no GPU): the shape key, the LRU bookkeeping (shape_cache.py) and the label padding of
lrs_data.collate_pad that keeps the number of shape keys of a bucketed LRS epoch small."""
import pytest
import torch

from syncvsr_amd.lrs_data import collate_pad
from syncvsr_amd.shape_cache import ShapeLRU, shape_key


def test_shape_key_shapes_dtypes_and_non_tensors():
    a = [torch.zeros(2, 9, 1, 24, 24), torch.zeros(2, dtype=torch.int32), None]
    assert shape_key(a) == shape_key([torch.ones(2, 9, 1, 24, 24), torch.ones(2, dtype=torch.int32), None])
    assert shape_key(a) != shape_key([torch.zeros(2, 10, 1, 24, 24), a[1], None])          # frames
    assert shape_key(a) != shape_key([a[0], torch.zeros(2, dtype=torch.int64), None])       # dtype
    assert shape_key(a) != shape_key([a[0][:1], a[1][:1], None])                            # batch (LRW's short last batch)
    assert shape_key(a) != shape_key([a[0], a[1], torch.zeros(2, 9)])                       # a slot present or not
    k = shape_key(a)
    assert hash(k) == hash(shape_key(a)) and k[2] == "NoneType"


def test_lru_order_and_count_bound():
    lru = ShapeLRU(2)
    assert lru.put("A", 1) == []
    assert lru.put("B", 2) == []
    assert lru.get("A") == 1                       # A becomes the most recently used
    assert lru.keys() == ["B", "A"]
    assert lru.put("C", 3) == [("B", 2)]           # B is the least recently used
    assert lru.keys() == ["A", "C"]
    assert lru.peek("A") == 1 and lru.keys() == ["A", "C"]       # peek does not touch the order
    assert lru.get("B") is None
    assert lru.put("C", 4) == [] and lru.peek("C") == 4          # replacing evicts nothing
    assert lru.pop_all() == [("A", 1), ("C", 4)] and len(lru) == 0
    with pytest.raises(ValueError):
        ShapeLRU(0)


def test_lru_sequence_of_the_gpu_eviction_test():
    """A B A C B A C A with two slots: every key comes back after its eviction (6 recordings), the order the GPU test relies on."""
    lru, recorded, evicted = ShapeLRU(2), [], []
    for s in "ABACBACA":
        if lru.get(s) is None:
            evicted += [k for k, _ in lru.put(s, True)]
            recorded.append(s)
    assert recorded == list("ABCBAC")
    assert evicted == list("BACB")
    assert lru.keys() == ["C", "A"]


def test_lru_weight_bound_keeps_the_newest():
    lru = ShapeLRU(8, max_weight=100, weight=lambda v: v)
    for k, w in (("A", 40), ("B", 40), ("C", 40)):
        lru.put(k, w)
    assert lru.shrink(keep="C") == [("A", 40)]
    assert lru.total_weight() == 80
    lru.put("D", 500)
    assert lru.shrink(keep="D") == [("B", 40), ("C", 40)]            # the one just recorded stays, even over the budget
    assert lru.keys() == ["D"]
    assert ShapeLRU(2).shrink() == []                                 # no weight bound: nothing to do


def _samples(frames, targets):
    return [{"input": torch.ones(t, 1, 4, 4), "target": torch.arange(1, n + 1)} for t, n in zip(frames, targets)]


@pytest.mark.parametrize("k,lens,want", [(16, (3, 7), 16), (16, (16,), 16), (16, (17, 1), 32), (4, (5, 2), 8), (1, (5, 2), 5)])
def test_collate_pad_targets_to_multiple(k, lens, want):
    out = collate_pad(_samples([5] * len(lens), lens), pad_targets_to_multiple=k)
    t = out["targets"]
    assert t.shape == (len(lens), 1, want)
    assert out["target_lengths"].tolist() == list(lens)                 # the real lengths
    for row, n in zip(t[:, 0], lens):
        assert row[:n].tolist() == list(range(1, n + 1)) and bool((row[n:] == -1).all())


def test_collate_pad_targets_and_frames_together():
    """Frame padding (the sampler's bucket bound) and label padding are independent axes: frames go to pad_frames_to, audio at its rate,
    targets to the multiple; without pad_targets_to_multiple the targets keep the longest transcript, as the reference does."""
    batch = _samples([5, 9], [3, 6])
    for b, n in zip(batch, (5, 9)):
        b["audio"] = torch.ones(n * 4, 2, dtype=torch.long)
    out = collate_pad(batch, pad_frames_to=16, frames_per_unit={"audio": 4}, pad_targets_to_multiple=16)
    assert out["inputs"].shape == (2, 16, 1, 4, 4) and out["input_lengths"].tolist() == [5, 9]
    assert out["audios"].shape == (2, 64, 2)
    assert out["targets"].shape == (2, 1, 16)
    plain = collate_pad(batch, pad_frames_to=16, frames_per_unit={"audio": 4})
    assert plain["targets"].shape == (2, 1, 6)
    assert torch.equal(out["targets"][:, :, :6], plain["targets"])
    assert torch.equal(out["inputs"], plain["inputs"])


def test_collate_pad_target_padding_rejects_bad_arguments():
    with pytest.raises(ValueError):
        collate_pad(_samples([5], [3]), pad_targets_to_multiple=0)
    with pytest.raises(ValueError):
        collate_pad(_samples([5], [3]), pad_frames_to=8, frames_per_unit={"target": 1}, pad_targets_to_multiple=4)

"""``resident.pack_parts``: what the one pinned copy of a resident batch carries -- the pick list
``[B]``, then the running offsets ``[B + 1]`` of every active view (model: the row bases; doc: the
doc-node and pair bases; eval: the word bases) -- is the parts end to end as int32, and the
returned slices recover each part exactly.  Every part holds values of its own, so a slice that
is shifted into a neighbouring part cannot pass."""
import numpy as np
import pytest

# the part lists batch() forms: no view; one view of one part (model, or eval alone); model + doc;
# model + doc + eval
LENGTHS = {"pick": lambda B: [B], "one_view": lambda B: [B, B + 1], "model_doc": lambda B: [B] + [B + 1] * 3,
           "all": lambda B: [B] + [B + 1] * 4}


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("name", sorted(LENGTHS))
def test_flat_is_the_parts_end_to_end_and_the_slices_recover_them(name, B):
    from hetersumgraph_amd.resident import pack_parts
    lengths = LENGTHS[name](B)
    parts = [1000 * (i + 1) + np.arange(n, dtype=np.int64) for i, n in enumerate(lengths)]
    flat, cuts = pack_parts(parts)
    assert flat.dtype == np.int32 and flat.shape == (sum(lengths),) and flat.flags["C_CONTIGUOUS"]
    assert flat.tolist() == [int(x) for a in parts for x in a]
    assert len(cuts) == len(parts)
    for a, c in zip(parts, cuts):
        assert isinstance(c, slice) and c.step in (None, 1)
        assert np.array_equal(flat[c], a) and flat[c].dtype == np.int32
    # the slices tile the array in order, with no gap and no overlap
    assert [c.start for c in cuts] == [0] + list(np.cumsum(lengths)[:-1]) and cuts[-1].stop == len(flat)

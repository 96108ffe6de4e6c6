"""The four counters of small launches of the frame kernels, pinned bit for bit to the values the parent build computed
(tests/golden/frame_counts_parent.npz, recorded by tests/golden/make_frame_counts_parent.py on an MI355X before the kernels' packed
fp32 arithmetic was written per component).  That change -- and any later one that promises the same IEEE operations on the same
operands in the same order -- leaves every counter of every case as it was: no tolerance.

Cases (tests/frame_counts_cases.py): the seven built geometries at N = 256, k = 4, and the same seven through the generic kernels;
wtx at k = 2 and 6; one plain geometry each at N = 64, 128, 512, 1024; an allocation; a masked N = 256 plan.  Each 2 SNR cells x 8
frames, from frame offset 0 and from an offset above 2^32."""
import numpy as np
import pytest

import frame_counts_cases as FC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pinned(golden):
    return golden("frame_counts_parent.npz")


def test_the_cases_the_file_holds(pinned):
    assert sorted(pinned.files) == sorted("%s/%d" % (n, off) for n in FC.CASES for off in FC.OFFSETS)
    assert len(FC.STRUCTURES) == 7 and FC.OFFSETS[0] == 0 and FC.OFFSETS[1] > 2 ** 32


@pytest.mark.parametrize("name", list(FC.CASES))
def test_counters_are_the_parent_builds(channels, pinned, name):
    got = FC.run_case(name, channels)
    for off, g in zip(FC.OFFSETS, got):
        want = pinned["%s/%d" % (name, off)]
        print("%s offset %d: bit errors %s (pinned %s)" % (name, off, g[..., 0].ravel(), want[..., 0].ravel()))
        assert g.dtype == want.dtype and g.shape == want.shape and g.shape[-1] == 4
        assert np.array_equal(g, want)
        assert g[..., 0].sum() > 0 and (g[..., 1] > 0).all()
    assert not np.array_equal(got[0][..., 0], got[1][..., 0])          # (other frames, other errors)

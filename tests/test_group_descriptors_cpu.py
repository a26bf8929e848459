"""The host's rule for a group launch's buffer descriptors (include/gffx_hip.h: gffx_hip_group_descriptors_fit):
a batch is served through descriptors of its whole buffers only while each spans at most 2^31 bytes -- a position must be a 32-bit
byte offset that cannot wrap, and the offset 2^31 (kWinNoLine, what a lane that must not write selects) must lie beyond every
buffer.  12 bytes per region, 4 per word of the pair buffer.  A pure function: no device, no allocation.
"""
import pytest

from gffx_amd import _ffi

LIMIT = 1 << 31


def fit(nq, cap, pair_out=1):
    return _ffi.lib().gffx_hip_group_descriptors_fit(int(nq), int(cap), int(pair_out))


def test_small_batches_take_the_descriptors():
    assert fit(1, 1024) == 1
    assert fit(1_000_000, 2_000_000) == 1
    assert fit(1, 0) == 1  # (a pair buffer of no words: an empty descriptor)


@pytest.mark.parametrize("words", [LIMIT // 4 - 1, LIMIT // 4])
def test_pair_buffer_up_to_the_limit(words):
    assert fit(1000, words) == 1


@pytest.mark.parametrize("words", [LIMIT // 4 + 1, (1 << 32) // 4 - 1, (1 << 32) // 4, (1 << 32) // 4 + 1, 1 << 40, (1 << 64) - 1])
def test_pair_buffer_beyond_the_limit_takes_the_per_round_descriptors(words):
    """... at 2^31 bytes + one word, around 2^32 bytes (where a byte offset no longer fits 32 bits at all) and far beyond"""
    assert fit(1000, words) == 0


def test_regions_at_the_limit():
    most = LIMIT // 12  # 12 bytes per region: three words, rows or columns
    assert most * 12 <= LIMIT < (most + 1) * 12
    assert fit(most, 1024) == 1
    assert fit(most + 1, 1024) == 0
    for nq in ((1 << 32) // 12, (1 << 32) // 12 + 1, 1 << 40):
        assert fit(nq, 1024) == 0


def test_a_pass_without_pair_output_ignores_the_capacity():
    """counts-only passes carry capacity = "no limit" in the record: it is not a buffer's size"""
    assert fit(1000, (1 << 64) - 1, 0) == 1
    assert fit(LIMIT // 12 + 1, 0, 0) == 0

"""Host side of the deterministic voxel binning and IWE splats (no GPU): the bit rule shared by every fixed-point sum -- its Python
mirror next to cm_det_scale_log2 against the definition, against the documented values at the boundary shapes and against the
library's evf_splat_det_bits -- and the choice of entry point the encodings make from the switch and the requested outputs."""

import pytest

from event_flow_amd import _lib
from event_flow_amd.dataloader import encodings as enc
from event_flow_amd.loss import flow as hloss

EVF_EINVAL, EVF_ENOTSUP = -22, -95


@pytest.fixture
def det_on():
    before = _lib.deterministic()
    _lib.set_deterministic(True)
    try:
        yield
    finally:
        _lib.set_deterministic(before)


def by_definition(terms, cbound):
    """the largest k with terms * cbound * 2^k < 2^62, searched"""
    k = 62
    while terms * cbound * 2 ** k >= 2 ** 62:
        k -= 1
    return k


def test_bit_rule_at_the_boundary_shapes():
    bits = hloss.splat_det_bits
    # the documented values: the loss at its benchmark shapes, a voxel grid / count image of 15000 events
    assert bits(15000, 10) == 44 and bits(50000, 1) == 46 and bits(15000, 1) == 48
    # the largest admitted terms x bound (k = 32) and the first refused one (k = 31), by either factor
    assert bits(2 ** 30 - 1, 1) == 32 and bits(2 ** 30, 1) == 31
    assert bits(2 ** 20, 2 ** 10 - 1) == 32 and bits(2 ** 20, 2 ** 10) == 31
    assert bits(1, 2 ** 30 - 64) == 32 and bits(1, 2 ** 30) == 31  # (the bound is a float32: 2^30 - 64 is the one below 2^30)
    assert hloss.CM_DET_MIN_LOG2 == 32
    # a bound below 1 counts as 1 (no term is allowed more bits than a count), a fractional one by its ceiling
    assert bits(5, 0.25) == bits(5, 1) == bits(5, 0) == 59
    assert bits(2 ** 20, 1022.5) == bits(2 ** 20, 1023) == 32 and bits(2 ** 20, 1023.5) == 31
    assert bits(1000, 2.000001) == bits(1000, 3)
    for terms in (1, 2, 3, 600, 1023, 1024, 15000, 2 ** 24 + 1, 2 ** 30 - 1, 2 ** 30):
        for bound in (1, 2, 3, 10, 1023, 1024):
            k = bits(terms, bound)
            assert k == by_definition(terms, bound), (terms, bound)
            assert terms * bound * 2 ** k < 2 ** 62 <= terms * bound * 2 ** (k + 1)
    # the loss's rule is this rule
    for M, P in ((15000, 10), (5, 0), (2 ** 20, 2 ** 10), (2 ** 30 - 1, 1)):
        assert hloss.cm_det_scale_log2(M, P) == bits(M, max(P, 1))


def test_library_agrees_with_the_mirror_and_refuses_below_32_bits():
    lib = _lib.load()
    for terms, bound in ((1, 1.0), (600, 1.0), (15000, 10.0), (15000, 0.25), (2 ** 30 - 1, 1.0), (2 ** 20, 1023.0), (2 ** 20, 1022.5),
                         (1, float(2 ** 30 - 64)), (7, 2.5)):
        assert lib.evf_splat_det_bits(terms, bound) == hloss.splat_det_bits(terms, bound) >= 32, (terms, bound)
    for terms, bound in ((2 ** 30, 1.0), (2 ** 20, 1024.0), (2 ** 20, 1023.5), (1, float(2 ** 30)), (2 ** 40, 1.0), (2 ** 62, 3e38)):
        assert hloss.splat_det_bits(terms, bound) < 32
        assert lib.evf_splat_det_bits(terms, bound) == EVF_ENOTSUP, (terms, bound)
    for terms, bound in ((0, 1.0), (-3, 1.0), (5, -1.0), (5, float("nan")), (5, float("inf"))):
        assert lib.evf_splat_det_bits(terms, bound) == EVF_EINVAL, (terms, bound)


def test_refusal_text_names_the_limit():
    assert _lib.splat_det_refusal(600, 1.0, 5, 3276, 1) is None  # 16380 slots per row
    assert "16384" in _lib.splat_det_refusal(600, 1.0, 5, 3277, 1)  # 16385
    assert "16384" in _lib.splat_det_refusal(600, 1.0, 1, 16385, 1)
    assert "2^30" in _lib.splat_det_refusal(2 ** 30, 1.0, 1, 8, 1)
    assert "2^30" in _lib.splat_det_refusal(2 ** 20, 1024.0, 4, 8, 1)
    assert "65535" in _lib.splat_det_refusal(10, 1.0, 1, 8, 65536)
    assert _lib.splat_det_refusal(0, 1.0, 1, 8, 1) is None  # no events: zero-filled outputs


def test_encodings_choose_the_entry_point_from_switch_and_outputs(det_on):
    pick = enc._encode_entry
    assert pick("evf_encode_events", True, 700, 5, 40, 2) == "evf_encode_events_det"
    assert pick("evf_encode_window", True, 700, 5, 40, 6) == "evf_encode_window_det"
    assert pick("evf_encode_events", False, 700, 5, 40, 2) == "evf_encode_events"  # cnt / mask / pol only: the default call
    assert pick("evf_encode_events", False, 2 ** 30, 5, 16385, 2) == "evf_encode_events"
    with pytest.raises(_lib.EvflowError, match="16384"):
        pick("evf_encode_events", True, 700, 5, 3277, 2)
    with pytest.raises(_lib.EvflowError, match="2\\^30"):
        pick("evf_encode_window", True, 2 ** 30, 2, 40, 2)
    _lib.set_deterministic(False)
    assert pick("evf_encode_events", True, 700, 5, 40, 2) == "evf_encode_events"
    assert pick("evf_encode_events", True, 700, 5, 3277, 2) == "evf_encode_events"  # (the default path has no such limit)

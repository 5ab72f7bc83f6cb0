"""Which packets of an rmx_step_seq window are private hand-offs (no release fence behind them), without a GPU.

rmx_seq_handoff is the rule the window recorder itself applies to every packet it records (csrc/rmx_internal.h
seq_handoff): packets 0 .. K - 2 of a packed window, never the last one, never a packet of an unpacked window
(RMX_SEQ_PACKED=0, ineligible handles) or of a one-step window, and none at all with RMX_SEQ_RELEASE=1."""
import pytest

from rmx import _capi


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library()


def marks(lib, K, packed, release_all=0):
    return [lib.rmx_seq_handoff(k, K, packed, release_all) for k in range(K)]


@pytest.mark.parametrize("K", [2, 3, 8, 64, 1100])
def test_packed_window_marks_all_but_the_last(lib, K):
    assert marks(lib, K, 1) == [1] * (K - 1) + [0]


@pytest.mark.parametrize("K", [1, 2, 3, 8, 64])
def test_unpacked_window_marks_none(lib, K):
    """RMX_SEQ_PACKED=0 and every ineligible handle record an unpacked window: every packet keeps its release."""
    assert marks(lib, K, 0) == [0] * K


def test_one_step_window_marks_none(lib):
    assert marks(lib, 1, 1) == [0] and marks(lib, 1, 0) == [0]


@pytest.mark.parametrize("K", [2, 7, 64])
def test_release_switch_marks_none(lib, K):
    """RMX_SEQ_RELEASE=1: the packed window's packets all keep their release fence."""
    assert marks(lib, K, 1, release_all=1) == [0] * K


def test_packets_outside_the_window_are_never_marked(lib):
    for K in (2, 7):
        assert lib.rmx_seq_handoff(-1, K, 1, 0) == 0
        assert lib.rmx_seq_handoff(K, K, 1, 0) == 0
        assert lib.rmx_seq_handoff(K - 1, K, 1, 0) == 0
    assert lib.rmx_seq_handoff(0, 0, 1, 0) == 0

"""CPU check of tests/packed_conv_ref.py, the float64 reference of the packed-conv GPU tests: a two-segment case worked out by hand."""
import numpy as np

from packed_conv_ref import packed_conv_ref64, seg_bounds


def test_packed_reference_against_a_hand_computed_two_segment_case():
    # one channel, segments [1, 2, 3] and [10, 20], taps (1, 10, 100) on (x[n - 1], x[n], x[n + 1]), bias 0.5: no tap crosses the boundary
    x = np.array([[1, 2, 3, 10, 20]], np.float32)
    w = np.array([[[1], [10], [100]]], np.float32)
    b = np.array([0.5], np.float32)
    y = packed_conv_ref64(x, [3, 2], w, b)
    want = [10 * 1 + 100 * 2, 1 * 1 + 10 * 2 + 100 * 3, 1 * 2 + 10 * 3, 10 * 10 + 100 * 20, 1 * 10 + 10 * 20]
    assert y.dtype == np.float64 and np.array_equal(y, np.array([want], np.float64) + 0.5)
    # dilation 2 ("same" padding 2): the 2-long segment is shorter than the halo, only its centre tap lands inside it
    y = packed_conv_ref64(x, [3, 2], w, None, dil=2)
    assert np.array_equal(y, np.array([[10 * 1 + 100 * 3, 10 * 2, 1 * 1 + 10 * 3, 10 * 10, 10 * 20]], np.float64))
    # leaky relu on the input first
    y = packed_conv_ref64(-x, [3, 2], np.array([[[0], [1], [0]]], np.float32), None, in_slope=0.5)
    assert np.array_equal(y, -0.5 * x.astype(np.float64))
    # transposed, stride 2, k = 4, padding 1: y[2 n + p] = sum_j w[p + 1 - 2 j ...]; by hand for the segment [1, 2] and the segment [5]
    xt = np.array([[1, 2, 5]], np.float32)
    wt = np.array([[[1], [10], [100], [1000]]], np.float32)       # out[i * 2 - 1 + t] += x[i] * w[t]
    y = packed_conv_ref64(xt, [2, 1], wt, None, stride_transposed=2)
    assert np.array_equal(y, np.array([[10 * 1, 100 * 1 + 1 * 2, 1000 * 1 + 10 * 2, 100 * 2, 10 * 5, 100 * 5]], np.float64))
    # depthwise: every channel with its own taps
    xd = np.array([[1, 2, 3], [4, 5, 6]], np.float32)
    wd = np.array([[[1], [0], [0]], [[0], [0], [1]]], np.float32)
    y = packed_conv_ref64(xd, [1, 2], wd, None, depthwise=True)
    assert np.array_equal(y, np.array([[0, 0, 2], [0, 6, 0]], np.float64))
    assert seg_bounds([3, 2], 4) == [(0, 12), (12, 20)]

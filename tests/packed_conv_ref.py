"""Float64 reference of a conv on utterances packed back to back along the time axis: every segment is convolved on its own (zero padding at
ITS edges -- that is the definition of correct for a packed batch) and the results are concatenated in the same order."""
import numpy as np


def seg_bounds(lengths, scale=1):
    off = np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))]) * scale
    return [(int(off[i]), int(off[i + 1])) for i in range(len(lengths))]


def packed_conv_ref64(x, lengths, w, bias, dil=1, stride_transposed=0, depthwise=False, in_slope=None):
    """x: [Cin, sum(lengths)] float32; w: [Cout, k, Cin] (depthwise: [C, k, 1]).  'Same' padding dil (k - 1) / 2, or a transposed conv with
    padding (k - stride) / 2.  in_slope: leaky relu applied to the input first.  Returns float64 [Cout, sum(lengths) * max(stride, 1)]."""
    import torch
    import torch.nn.functional as F
    assert x.shape[1] == int(np.sum(lengths))
    k = w.shape[1]
    xt = torch.from_numpy(np.ascontiguousarray(x)).double()
    if in_slope is not None:
        xt = torch.where(xt < 0, xt * float(np.float32(in_slope)), xt)
    wt = torch.from_numpy(np.ascontiguousarray(w)).double()
    bt = None if bias is None else torch.from_numpy(np.ascontiguousarray(bias)).double()
    out = []
    for lo, hi in seg_bounds(lengths):
        s = xt[None, :, lo:hi]
        if stride_transposed:
            y = F.conv_transpose1d(s, wt.permute(2, 0, 1).contiguous(), bt, stride=stride_transposed, padding=(k - stride_transposed) // 2)
        elif depthwise:
            y = F.conv1d(s, wt.permute(0, 2, 1).contiguous(), bt, padding=dil * (k - 1) // 2, dilation=dil, groups=x.shape[0])
        else:
            y = F.conv1d(s, wt.permute(0, 2, 1).contiguous(), bt, padding=dil * (k - 1) // 2, dilation=dil)
        assert y.shape[2] == (hi - lo) * max(stride_transposed, 1)
        out.append(y[0])
    return torch.cat(out, dim=1).numpy()

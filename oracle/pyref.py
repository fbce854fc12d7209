"""ctypes bindings for the parity checkers.  TEST INFRASTRUCTURE ONLY.

Only ``tests/``, ``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline`` leg may import this
module; the product (``summertts_amd``) never does.

Two checkers share one Python interface (``RefModel`` / ``PortModel``):

* ``oracle/_ref/libsummertts_ref.so`` -- the real SummerTTS Eigen path, compiled in place from
  /root/reference by ``oracle/Makefile`` and driven by ``oracle/ref_harness.cpp``.
* ``oracle/libvits_oracle.so`` -- the plain-C restatement ``oracle/vits_oracle.c``.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Dict, Optional, Sequence

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SO = os.path.join(HERE, "_ref", "libsummertts_ref.so")
PORT_SO = os.path.join(HERE, "libvits_oracle.so")
REFERENCE_ROOT = "/root/reference"


# The checkers parallelise with OpenMP.  On a many-core host (the GPU box: 256 CPUs) libgomp's default -- one thread per CPU, each spinning
# between parallel regions -- turns a tiny model's thousands of short loops into minutes of wall time and ~16 cores of pure spinning next
# to the HIP runtime's own threads (round 6: tests/fake_rccl/three_ranks.py took 8 m 45 s of a 12-minute GPU suite, 137 CPU-minutes).  The
# team is capped at 16 threads when the first model is created (omp_set_num_threads: works whether or not libgomp is already loaded), unless
# the user chose OMP_NUM_THREADS; bench.py's cpu_baseline leg sets the team size it measures with explicitly afterwards.
_omp_capped = False


def _cap_omp_threads() -> None:
    global _omp_capped
    if _omp_capped or os.environ.get("OMP_NUM_THREADS"):
        return
    _omp_capped = True
    for name in ("libgomp.so.1", "libgomp.so"):
        try:
            C.CDLL(name, mode=C.RTLD_GLOBAL).omp_set_num_threads(int(min(16, os.cpu_count() or 1)))
            return
        except OSError:
            continue


def build(port: bool = True, ref: bool = True, quiet: bool = True) -> None:
    """Compile the checkers (ref only when /root/reference exists: it does not on the GPU box)."""
    targets = []
    if port:
        targets.append("port")
    if ref and os.path.isdir(REFERENCE_ROOT):
        targets.append("ref")
    if targets:
        subprocess.run(["make", "-C", HERE, "-j8"] + targets, check=True,
                       stdout=subprocess.DEVNULL if quiet else None)


def have_ref() -> bool:
    return os.path.exists(REF_SO)


def have_port() -> bool:
    return os.path.exists(PORT_SO)


class _Model:
    """Common wrapper: both libraries export the same C symbols with a prefix."""

    TAPS = ("x_enc", "m", "logs", "logw", "z_p", "z")

    def __init__(self, so: str, prefix: str, blob: np.ndarray):
        self.lib = C.CDLL(so)
        _cap_omp_threads()
        self.p = prefix
        f = self._f
        f("create").restype = C.c_void_p
        f("create").argtypes = [C.c_void_p, C.c_int64]
        f("consumed").restype = C.c_int64
        f("consumed").argtypes = [C.c_void_p]
        f("speaker_num").restype = C.c_int
        f("speaker_num").argtypes = [C.c_void_p]
        f("destroy").argtypes = [C.c_void_p]
        f("infer_ids").restype = C.c_int64
        f("infer_ids").argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_int]
        f("wave").restype = C.POINTER(C.c_float)
        f("wave").argtypes = [C.c_void_p]
        f("durations").restype = C.POINTER(C.c_int32)
        f("durations").argtypes = [C.c_void_p]
        f("pcm").argtypes = [C.c_void_p, C.c_void_p]
        f("tap").restype = C.c_int
        f("tap").argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.POINTER(C.c_float)),
                             C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        f("times").argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        self.blob = np.ascontiguousarray(blob, dtype=np.float32)
        self.h = f("create")(self.blob.ctypes.data, self.blob.size)
        if not self.h:
            raise RuntimeError("oracle: model construction failed")

    def _f(self, name):
        return getattr(self.lib, self.p + name)

    @property
    def consumed(self) -> int:
        return int(self._f("consumed")(self.h))

    @property
    def speaker_num(self) -> int:
        return int(self._f("speaker_num")(self.h))

    def infer_ids(self, ids: Sequence[int], sid: int = 0, length_scale: float = 1.0,
                  forced_dur: Optional[Sequence[int]] = None, taps: bool = False) -> Dict[str, np.ndarray]:
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        fd = None
        if forced_dur is not None:
            fd = np.ascontiguousarray(forced_dur, dtype=np.int32)
            assert fd.size == ids.size
        n = int(self._f("infer_ids")(self.h, ids.ctypes.data, ids.size, sid, length_scale,
                                       fd.ctypes.data if fd is not None else None, 1 if taps else 0))
        wave = np.ctypeslib.as_array(self._f("wave")(self.h), shape=(n,)).copy()
        dur = np.ctypeslib.as_array(self._f("durations")(self.h), shape=(ids.size,)).copy()
        pcm = np.empty(n, np.int16)
        self._f("pcm")(self.h, pcm.ctypes.data)
        tm = (C.c_double * 5)()
        self._f("times")(self.h, tm)
        out = {"wave": wave, "durations": dur, "pcm": pcm,
               "times": dict(zip(("te", "dp", "flow", "dec", "total"), list(tm)))}
        if taps:
            for name in self.TAPS:
                ptr = C.POINTER(C.c_float)()
                r, c = C.c_int32(), C.c_int32()
                if self._f("tap")(self.h, name.encode(), C.byref(ptr), C.byref(r), C.byref(c)) == 0:
                    # column-major [rows=time, cols=channels]  ->  numpy [channels, time]
                    out[name] = np.ctypeslib.as_array(ptr, shape=(c.value, r.value)).copy()
        return out

    def close(self):
        if self.h:
            self._f("destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_port_lib = None


def _port():
    global _port_lib
    if _port_lib is None:
        if not have_port():
            build(port=True, ref=False)
        lib = C.CDLL(PORT_SO)
        lib.port_attention.restype = None
        lib.port_attention.argtypes = [C.c_void_p] * 5 + [C.c_int32] * 4 + [C.c_void_p]
        lib.port_layer_norm.restype = None
        lib.port_layer_norm.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
        lib.port_resblock_layer.restype = None
        lib.port_resblock_layer.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                            C.c_int32, C.c_float]
        lib.port_wn_layer.restype = None
        lib.port_wn_layer.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int32]
        lib.port_dds_layer.restype = None
        lib.port_dds_layer.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 6
        lib.port_convflow_step.restype = None
        lib.port_convflow_step.argtypes = ([C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 6 + [C.c_int32] * 3 + [C.c_void_p] * 8 +
                                           [C.c_float] + [C.c_void_p] * 4)
        lib.port_oproj_ln.restype = None
        lib.port_oproj_ln.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 6
        _port_lib = lib
    return _port_lib


def port_attention(q, k, v, relk, relv, nheads: int, win: int, lengths) -> np.ndarray:
    """The oracle's attention loop (vits_oracle.c attention_core, what mha_forward runs between its convs) on a packed batch: q, k, v
    float32 [nheads * kc][sum(lengths)], relk / relv [kc][2 win + 1] or None with win = 0 -> float32, every utterance on its own."""
    lib = _port()
    q = np.ascontiguousarray(q, dtype=np.float32)
    k = np.ascontiguousarray(k, dtype=np.float32)
    v = np.ascontiguousarray(v, dtype=np.float32)
    rows = q.shape[0]
    kc = rows // nheads
    assert rows == nheads * kc and k.shape == q.shape and v.shape == q.shape and int(np.sum(lengths)) == q.shape[1]
    if win > 0:
        relk = np.ascontiguousarray(relk, dtype=np.float32)
        relv = np.ascontiguousarray(relv, dtype=np.float32)
        assert relk.shape == (kc, 2 * win + 1) and relv.shape == relk.shape
    out = np.zeros(q.shape, np.float32)
    off = 0
    for n in lengths:
        n = int(n)
        part = [np.ascontiguousarray(x[:, off:off + n]) for x in (q, k, v)]
        o = np.zeros((rows, n), np.float32)
        lib.port_attention(part[0].ctypes.data, part[1].ctypes.data, part[2].ctypes.data, relk.ctypes.data if win > 0 else None,
                           relv.ctypes.data if win > 0 else None, nheads, kc, win, n, o.ctypes.data)
        out[:, off:off + n] = o
        off += n
    return out


def port_layer_norm(x, gamma, beta, post_gelu: bool = False) -> np.ndarray:
    """The oracle's LayerNorm over channels (vits_oracle.c layer_norm, then act_gelu when asked) of x float32 [C][T] -> float32 [C][T]."""
    lib = _port()
    y = np.array(x, dtype=np.float32, order="C", copy=True)
    g = np.ascontiguousarray(gamma, dtype=np.float32)
    b = np.ascontiguousarray(beta, dtype=np.float32)
    assert y.ndim == 2 and g.shape == (y.shape[0],) and b.shape == g.shape
    lib.port_layer_norm(y.ctypes.data, y.shape[0], y.shape[1], g.ctypes.data, b.ctypes.data, 1 if post_gelu else 0)
    return y


def port_resblock_layer(x, lengths, w1, b1, dil1: int, w2, b2, slope: float) -> np.ndarray:
    """The oracle's ResBlock layer x + conv2(lrelu(conv1_dil(lrelu(x)))) (vits_oracle.c resblock_layer, what resblock_forward loops over) on a
    packed batch: x float32 [C][sum(lengths)], w1 [C][k1][C], w2 [C][k2][C], b1 / b2 [C] or None -> float32, every utterance on its own."""
    lib = _port()
    x = np.ascontiguousarray(x, dtype=np.float32)
    w1 = np.ascontiguousarray(w1, dtype=np.float32)
    w2 = np.ascontiguousarray(w2, dtype=np.float32)
    b1 = None if b1 is None else np.ascontiguousarray(b1, dtype=np.float32)
    b2 = None if b2 is None else np.ascontiguousarray(b2, dtype=np.float32)
    Cc = x.shape[0]
    assert x.ndim == 2 and int(np.sum(lengths)) == x.shape[1] and w1.ndim == 3 and w2.ndim == 3
    assert w1.shape[0] == Cc and w1.shape[2] == Cc and w2.shape[0] == Cc and w2.shape[2] == Cc and w1.shape[1] % 2 == 1 and w2.shape[1] % 2 == 1
    assert (b1 is None or b1.shape == (Cc,)) and (b2 is None or b2.shape == (Cc,))
    out = np.zeros(x.shape, np.float32)
    off = 0
    for n in lengths:
        n = int(n)
        part = np.array(x[:, off:off + n], dtype=np.float32, order="C", copy=True)
        lib.port_resblock_layer(part.ctypes.data, Cc, n, w1.ctypes.data, None if b1 is None else b1.ctypes.data, w1.shape[1], int(dil1),
                                w2.ctypes.data, None if b2 is None else b2.ctypes.data, w2.shape[1], float(slope))
        out[:, off:off + n] = part
        off += n
    return out


def port_wn_layer(x, out, lengths, in_w, in_b, dil: int, rs_w, rs_b, g2=None):
    """The oracle's WaveNet layer (vits_oracle.c wn_layer, what wn_forward loops over) on a packed batch: gate = tanh . sigmoid of the in conv
    (+ g2 [2 H, B], the utterances' conditioning), then the 1x1 res / skip conv: rs_w [2 H][1][H] -> (x + rs[:H], out + rs[H:]); rs_w [H][1][H]
    (the last layer) -> (x, out + rs).  x, out float32 [H][sum(lengths)] -> the updated pair, every utterance on its own."""
    lib = _port()
    f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
    x, out, in_w, in_b, rs_w, rs_b, g2 = f(x), f(out), f(in_w), f(in_b), f(rs_w), f(rs_b), f(g2)
    H = x.shape[0]
    assert out.shape == x.shape and int(np.sum(lengths)) == x.shape[1] and in_w.shape[0] == 2 * H and in_w.shape[2] == H and in_w.shape[1] % 2 == 1
    assert rs_w.shape in ((H, 1, H), (2 * H, 1, H)) and (g2 is None or g2.shape == (2 * H, len(lengths)))
    xo, oo = np.zeros_like(x), np.zeros_like(out)
    off = 0
    for b, n in enumerate(lengths):
        n = int(n)
        px = np.array(x[:, off:off + n], dtype=np.float32, order="C", copy=True)
        po = np.array(out[:, off:off + n], dtype=np.float32, order="C", copy=True)
        gb = None if g2 is None else np.ascontiguousarray(g2[:, b])
        lib.port_wn_layer(px.ctypes.data, po.ctypes.data, H, n, in_w.ctypes.data, None if in_b is None else in_b.ctypes.data, in_w.shape[1], int(dil),
                          rs_w.ctypes.data, None if rs_b is None else rs_b.ctypes.data, None if gb is None else gb.ctypes.data,
                          1 if rs_w.shape[0] == H else 0)
        xo[:, off:off + n], oo[:, off:off + n] = px, po
        off += n
    return xo, oo


def _opt(a, shape=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float32)
    assert shape is None or a.shape == tuple(shape), (a.shape, shape)
    return a


def _ptr(a):
    return None if a is None else a.ctypes.data


def _dw_blob(dw_w, Cc):
    """[k][C] (the kernel entry's order) -> the blob's [C][k][1]."""
    dw_w = np.ascontiguousarray(dw_w, dtype=np.float32)
    assert dw_w.ndim == 2 and dw_w.shape[1] == Cc
    return np.ascontiguousarray(dw_w.T), dw_w.shape[0]


def port_dds_layer(x, lengths, dw_w, dw_b, dil: int, pad: int, g1, b1, w, bias, g2, b2) -> np.ndarray:
    """The oracle's DDSConv layer x + gelu(LN2(conv1x1(gelu(LN1(dwconv(x)))))) (vits_oracle.c dds_layer, what dds_forward loops over) on a
    packed batch: x float32 [C][sum(lengths)], dw_w [k][C] with ``pad`` zeros on the left and dil (k - 1) - pad on the right, w [C][C] in
    [out][in] order; dw_b / bias [C] or None -> float32, every utterance on its own."""
    lib = _port()
    x = np.ascontiguousarray(x, dtype=np.float32)
    Cc = x.shape[0]
    assert x.ndim == 2 and int(np.sum(lengths)) == x.shape[1]
    dw, k = _dw_blob(dw_w, Cc)
    assert 0 <= pad <= dil * (k - 1)
    dw_b, bias = _opt(dw_b, (Cc,)), _opt(bias, (Cc,))
    g1, b1, g2, b2 = (_opt(v, (Cc,)) for v in (g1, b1, g2, b2))
    w = _opt(w, (Cc, Cc))
    out = np.zeros(x.shape, np.float32)
    off = 0
    for n in lengths:
        n = int(n)
        part = np.array(x[:, off:off + n], dtype=np.float32, order="C", copy=True)
        lib.port_dds_layer(part.ctypes.data, Cc, n, dw.ctypes.data, _ptr(dw_b), k, int(dil), int(pad), g1.ctypes.data, b1.ctypes.data,
                           w.ctypes.data, _ptr(bias), g2.ctypes.data, b2.ctypes.data)
        out[:, off:off + n] = part
        off += n
    return out


def port_convflow_step(g, lengths, pre_w, pre_b, x0, x1, dw_w, dw_b, dil: int, pad: int, g1, b1, w, bias, g2, b2, proj_w=None, proj_b=None,
                       filter_sqrt: float = 1.0, with_input: bool = False):
    """The body of the oracle's convflow_inverse around one DDSConv layer, with sdp_forward's channel flip (vits_oracle.c
    port_convflow_step): h = conv1d(pre)(x0) + g, the layer, then (``proj_w`` [29][C] given) the projection and the inverse spline of x1
    per column.  g float32 [C][sum(lengths)], pre_w [C], pre_b [C] or None, x0 / x1 [sum(lengths)] or None (zeros).
    -> (y [C][L] the layer's output, o0 [L] or None, o1 [L] or None), every utterance on its own; ``with_input``: h [C][L] in front."""
    lib = _port()
    g = np.ascontiguousarray(g, dtype=np.float32)
    Cc, L = g.shape
    assert int(np.sum(lengths)) == L
    dw, k = _dw_blob(dw_w, Cc)
    assert 0 <= pad <= dil * (k - 1)
    pre_w, pre_b, dw_b, bias = _opt(pre_w, (Cc,)), _opt(pre_b, (Cc,)), _opt(dw_b, (Cc,)), _opt(bias, (Cc,))
    g1, b1, g2, b2 = (_opt(v, (Cc,)) for v in (g1, b1, g2, b2))
    w = _opt(w, (Cc, Cc))
    x0, x1 = _opt(x0, (L,)), _opt(x1, (L,))
    proj_w, proj_b = _opt(proj_w, (29, Cc)), _opt(proj_b, (29,))
    y, h = np.zeros((Cc, L), np.float32), np.zeros((Cc, L), np.float32)
    o0 = o1 = None
    if proj_w is not None:
        o0, o1 = np.zeros(L, np.float32), np.zeros(L, np.float32)
    off = 0
    for n in lengths:
        n = int(n)
        gp = np.ascontiguousarray(g[:, off:off + n])
        yp, hp, a0, a1 = np.zeros((Cc, n), np.float32), np.zeros((Cc, n), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
        p0 = None if x0 is None else np.ascontiguousarray(x0[off:off + n])
        p1 = None if x1 is None else np.ascontiguousarray(x1[off:off + n])
        lib.port_convflow_step(gp.ctypes.data, Cc, n, pre_w.ctypes.data, _ptr(pre_b), _ptr(p0), _ptr(p1), dw.ctypes.data, _ptr(dw_b), k,
                               int(dil), int(pad), g1.ctypes.data, b1.ctypes.data, w.ctypes.data, _ptr(bias), g2.ctypes.data,
                               b2.ctypes.data, _ptr(proj_w), _ptr(proj_b), float(filter_sqrt), hp.ctypes.data, yp.ctypes.data, a0.ctypes.data,
                               a1.ctypes.data)
        y[:, off:off + n], h[:, off:off + n] = yp, hp
        if proj_w is not None:
            o0[off:off + n], o1[off:off + n] = a0, a1
        off += n
    return (h, y, o0, o1) if with_input else (y, o0, o1)


def port_oproj_ln(att, w, bias, x, gamma, beta) -> np.ndarray:
    """The oracle's LN(x + conv1x1(att)) (vits_oracle.c text_encoder: the attention output projection, its residual and LayerNorm) of att
    float32 [C][T], w [C][C] in [out][in] order; bias [C] / x [C][T] or None -> float32 [C][T].  (Per column: no utterance boundaries.)"""
    lib = _port()
    att = np.ascontiguousarray(att, dtype=np.float32)
    Cc, T = att.shape
    w, bias, x = _opt(w, (Cc, Cc)), _opt(bias, (Cc,)), _opt(x, (Cc, T))
    gamma, beta = _opt(gamma, (Cc,)), _opt(beta, (Cc,))
    y = np.zeros((Cc, T), np.float32)
    lib.port_oproj_ln(att.ctypes.data, Cc, T, w.ctypes.data, _ptr(bias), _ptr(x), gamma.ctypes.data, beta.ctypes.data, y.ctypes.data)
    return y


class RefModel(_Model):
    """The real reference (Eigen CPU) acoustic path."""

    def __init__(self, blob: np.ndarray):
        if not have_ref():
            raise FileNotFoundError(REF_SO + " (run `make -C oracle ref` where /root/reference exists)")
        super().__init__(REF_SO, "ref_", blob)


class PortModel(_Model):
    """The plain-C restatement."""

    def __init__(self, blob: np.ndarray):
        if not have_port():
            build(port=True, ref=False)
        super().__init__(PORT_SO, "port_", blob)

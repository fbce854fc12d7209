"""NumPy statement of the speaker blend (include/summertts_hip.h sts_set_speaker_mix): for every channel the float64 sum, in term order, of
the float64 products weight[k] * E[sid[k]][c] (each exact: two fp32 factors), then the optional vector term, then ONE rounding to float32.
Tables are in the blob's layout, float32 [gin][speaker_num]; a mix is None (the plain sid) or a mapping with any of ``sid`` + ``weight``,
``vector`` and ``vector_weight`` (default 1), as ``Synthesizer.set_speaker_mix`` takes it."""
import numpy as np

MAX_TERMS = 16
MAX_WEIGHT = 16.0


def is_empty(mix) -> bool:
    return not mix or (len(mix.get("sid", ())) == 0 and mix.get("vector") is None)


def blend(table, mix, sid: int = 0) -> np.ndarray:
    """-> float32 [gin]: the conditioning vector of one utterance.  An empty mix takes row ``sid`` (outside the table -> 0, as a plain call)."""
    table = np.asarray(table, np.float32)
    gin, spk = table.shape
    if is_empty(mix):
        return table[:, sid if 0 <= sid < spk else 0].copy()
    acc = np.zeros(gin, np.float64)
    for s, w in zip(mix.get("sid", ()), mix.get("weight", ())):
        acc = acc + np.float64(np.float32(w)) * table[:, int(s)].astype(np.float64)       # (exact products, one float64 rounding per sum)
    if mix.get("vector") is not None:
        acc = acc + np.float64(np.float32(mix.get("vector_weight", 1.0))) * np.asarray(mix["vector"], np.float32).astype(np.float64)
    return acc.astype(np.float32)                                                        # (round to nearest even)


def blend_batch(table, mixes, sid=None) -> np.ndarray:
    """-> float32 [B][gin]"""
    return np.stack([blend(table, m, 0 if sid is None else int(sid[b])) for b, m in enumerate(mixes)])


def valid(speaker_num: int, gin: int, mix) -> bool:
    """the rules of sts_speaker_mix_check for one entry (speaker_num 0: a single-speaker model)"""
    if mix is None:
        return True
    sid, w = list(mix.get("sid", ())), list(mix.get("weight", ()))
    if len(sid) != len(w) or len(sid) > MAX_TERMS:
        return False
    if is_empty(mix):
        return True
    if speaker_num <= 0 or gin <= 0:
        return False
    ok_w = lambda x: bool(np.isfinite(np.float32(x))) and abs(float(np.float32(x))) <= MAX_WEIGHT
    if any(not 0 <= int(s) < speaker_num for s in sid) or any(not ok_w(x) for x in w):
        return False
    if mix.get("vector") is not None:
        v = np.asarray(mix["vector"], np.float32)
        if v.size != gin or not np.isfinite(v).all() or not ok_w(mix.get("vector_weight", 1.0)):
            return False
    return True


def blob_tail(blob, speaker_num: int, gin: int):
    """-> (head floats, table [gin][speaker_num]) of a multi-speaker blob, which ends with its speaker section (synth_blob.make_blob: the
    two counts as float values, then the table)."""
    blob = np.ascontiguousarray(blob, np.float32)
    pos = blob.size - speaker_num * gin - 2
    assert pos > 0 and blob[pos] == speaker_num and blob[pos + 1] == gin, "no speaker section of that size at the end of the blob"
    return blob[:pos].copy(), blob[pos + 2:].reshape(gin, speaker_num).copy()


def blob_with_extra_speakers(blob, speaker_num: int, gin: int, columns) -> np.ndarray:
    """blob B of the bit-for-bit yardstick: the same model with ``columns`` (float32 [m][gin]) appended to its speaker table as rows
    speaker_num .. speaker_num + m - 1"""
    head, table = blob_tail(blob, speaker_num, gin)
    cols = np.asarray(columns, np.float32).reshape(-1, gin)
    table_b = np.ascontiguousarray(np.concatenate([table, cols.T], axis=1), np.float32)
    hdr = np.asarray([speaker_num + cols.shape[0], gin], np.float32)
    return np.concatenate([head, hdr, table_b.ravel()]).astype(np.float32)

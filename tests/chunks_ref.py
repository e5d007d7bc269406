"""numpy statement of include/sqg_chunks.h: what sqg_batch_chunks must produce, bit for bit.  Written from the rules, sorting with
np.sort; no call into the library."""
import numpy as np

_CODE = np.ones(256, np.uint8)                      # src/seq.h:14-27: rank 0/1/2/3 -> 1/2/3/4; anything unknown is rank 0
for _letters, _c in ((b"CcYB", 2), (b"GgSK", 3), (b"TtU", 4)):
    for _b in _letters:
        _CODE[_b] = _c
_CODE_METH = _CODE.copy()
_CODE_METH[ord("M")] = 5


def stats(raw):
    """(med2, mad4): twice the median, four times the median absolute deviation, exact integers"""
    n = len(raw)
    if n == 0:
        return 0, 0
    s = np.sort(raw.astype(np.int64))
    med2 = int(s[(n - 1) // 2] + s[n // 2])
    d = np.sort(np.abs(2 * raw.astype(np.int64) - med2))
    return med2, int(d[(n - 1) // 2] + d[n // 2])


def n_chunks_of(n, L, S):
    return (n - L) // S + 1 if n >= L else 0


def normalise(raw, med2, mad4, norm, offset, rng, dig):
    if norm == "pa":
        return ((raw.astype(np.float64) + np.float64(offset)) * np.float64(rng) / np.float64(dig)).astype(np.float32)
    madp = mad4 / 4.0 if mad4 > 0 else 1.0
    inv = np.float32(1.0 / (1.4826 * madp))
    return ((raw.astype(np.float32) - np.float32(med2 / 2.0)) * inv).astype(np.float32)


def read_chunks(raw, ss, seq, k, rna, meth, L, S, W, dtype="f16", norm="medmad", offset=0.0, rng=1.0, dig=1.0):
    """one read -> dict(med2, mad4, signal [nc, L], labels [nc, W], label_len [nc], chunk_start [nc])"""
    raw = np.asarray(raw, np.int16)
    n = len(raw)
    med2, mad4 = stats(raw)
    nc = n_chunks_of(n, L, S) if len(seq) >= k else 0
    x = normalise(raw, med2, mad4, norm, offset, rng, dig)
    if dtype == "f16":
        x = x.astype(np.float16)
    sig = np.zeros((nc, L), x.dtype)
    lab = np.zeros((nc, W), np.uint8)
    ll = np.zeros(nc, np.int32)
    E = np.concatenate(([0], np.cumsum(np.asarray(ss, np.int64))))[:-1]          # first sample of every event, generation order
    codes = (_CODE_METH if meth else _CODE)[np.frombuffer(bytes(seq), np.uint8)]
    for j in range(nc):
        s = j * S
        sig[j] = x[s:s + L]
        g0, g1 = (n - s - L, n - s) if rna else (s, s + L)
        e0, e1 = int(np.searchsorted(E, g0, "left")), int(np.searchsorted(E, g1, "left"))
        ev = np.arange(e0, e1)
        if rna:
            ev = ev[::-1]
        ll[j] = e1 - e0
        m = min(e1 - e0, W)
        lab[j, :m] = codes[ev[:m]]
    return dict(med2=med2, mad4=mad4, signal=sig, labels=lab, label_len=ll, chunk_start=np.arange(nc, dtype=np.int64) * S)


def batch_chunks(reads, k, rna, meth, L, S, W, dtype="f16", norm="medmad", rng=1.0, dig=1.0):
    """reads: list of dict(sig, ss, seq, offset) -> the batch's outputs as sqg_chunk_out_t lays them out"""
    per = [read_chunks(r["sig"], r["ss"], r["seq"], k, rna, meth, L, S, W, dtype, norm, r.get("offset", 0.0), rng, dig) for r in reads]
    cat = lambda key, empty: np.concatenate([p[key] for p in per]) if per else empty       # noqa: E731
    return dict(signal=cat("signal", None), labels=cat("labels", None), label_len=cat("label_len", None),
                chunk_start=cat("chunk_start", None),
                chunk_read=np.concatenate([np.full(len(p["label_len"]), i, np.int32) for i, p in enumerate(per)]),
                med2=np.array([p["med2"] for p in per], np.int32), mad4=np.array([p["mad4"] for p in per], np.int32),
                chunk_off=np.concatenate(([0], np.cumsum([len(p["label_len"]) for p in per]))).astype(np.int64))


def bits(a):
    """floats as the integers of their bytes: -0 and NaN cannot hide in a comparison"""
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a

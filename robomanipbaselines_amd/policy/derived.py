"""One cache for values derived from parameters (packed GEMM planes, filter transforms, widened or
summed biases, padded heads): every policy network keeps them through `derived`."""


def _sig(t):
    return None if t is None else (t.data_ptr(), t._version, t.dtype, t.device, t.shape)


def derived(owner, slot, sources, build, extra=()):
    """build(), cached on `owner` under `slot`; rebuilt when a tensor of `sources` (None = an absent
    one) changes its (data_ptr, _version, dtype, device, shape), or when `extra` changes.  A hit
    compares host-side tuples only: no device work, no allocation, no sync.  In-place updates
    (copy_, load_state_dict, an optimizer step) bump the version and are seen; the one known limit:
    a write through `.data` or a `.detach()`ed alias bumps no version and is not."""
    key = (tuple(_sig(t) for t in sources), extra)
    cache = owner.__dict__.setdefault("_derived", {})
    ent = cache.get(slot)
    if ent is None or ent[0] != key:
        ent = cache[slot] = (key, build())
    return ent[1]

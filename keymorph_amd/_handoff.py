"""The one side-channel between operators: values that ride on a tensor OBJECT from the pass that produced the tensor to the
pass that consumes it, each guarded by the tensor's version counter.

    stats       (N,C,2) float64 (sum, sum^2) per (n, channel), from the epilogue that wrote the tensor
    grad_scale  device float[2] {S, 1/S}: the f16x3 range scale of a gradient
    layout      1 = fp32 channel-blocked (N, C/8, D, H, W, 8); 2 = pre-split records (N, C/8, V + 1, 8 floats = 8 fp16 hi + 8 fp16
                lo, what kmh_maxpool3d_bwd_split writes); 3 = pooled + winners: the pooled gradient (N,D/2,H/2,W/2,C) itself, which with
                the pooling operator's winner bytes stands for its scatter; absent = dense (N,D,H,W,C)
    lazy_gn     (c123, x): a GroupNorm backward still to be applied to this normalised-input gradient
    up_sources  (skip, low, skip_version, low_version) on the output of upcat()
    packed      (terms, wscale) on a packed-weight buffer

A payload is void once the tensor was modified in place; another tensor object (clone, detach, a view, what a hook returns, the
sum autograd forms of two gradients) carries nothing.  Where a lost or unexpected payload would be silently wrong (scrambled
channels, a GroupNorm backward applied twice or never) the consumer calls expect().  Needs torch only for `_version`."""
KEYS = ("stats", "grad_scale", "layout", "lazy_gn", "up_sources", "packed")
_ATTR = "_kmh_handoff"           # ONE attribute of the tensor object: {key: (payload, version at attach)}


def attach(t, key: str, payload) -> None:
    assert key in KEYS and payload is not None, key
    if not hasattr(t, _ATTR):
        setattr(t, _ATTR, {})
    getattr(t, _ATTR)[key] = (payload, t._version)


def peek(t, key: str):
    """the payload, or None when nothing was attached or the tensor changed since"""
    assert key in KEYS, key
    tag = getattr(t, _ATTR, {}).get(key)
    return tag[0] if (tag is not None and tag[1] == t._version) else None


def expect(t, key: str, present: bool, what: str, remedy: str) -> None:
    if (peek(t, key) is not None) != present:
        raise RuntimeError("keymorph_amd: %s: the tensor that arrived carries %s '%s' hand-off where %s was expected (a hook, "
                           "retain_grad, an in-place op or a second consumer replaced or changed it?) -- set %s=1"
                           % (what, "a" if not present else "no valid", key, "one" if present else "none", remedy))

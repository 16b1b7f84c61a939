"""The loss terms of lae_composite_rays_train_step for the tests that call the entry directly (include/laenerf.h: four structs, each
passed by reference or as NULL for an absent term)."""


def term_refs(depth=None, dist=None, crit=None, weight=None):
    """the entry's four term arguments: each term None (absent) or the field values of its struct in the header's order"""
    import ctypes

    from laenerf_amd import _lib
    classes = (_lib.DepthTerm, _lib.DistTerm, _lib.CritTerm, _lib.WeightTerm)
    return [None if v is None else ctypes.byref(cls(*v)) for cls, v in zip(classes, (depth, dist, crit, weight))]


def null_step(step, N=4, **terms):
    """the return code of the entry on base arguments that are all NULL (M = 8, N rays) plus these terms: -3 is what a valid call on
    NULL buffers gives, so -1 and 0 show what is checked before the pointers"""
    base = [None] * 4 + [8, N, 1e-4, None, None, None, 1.0, 1.0, 1.0] + [None] * 13 + [0]
    return step(*base, *term_refs(**terms), None)

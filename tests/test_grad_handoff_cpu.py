"""The argument checks of the field backward's hand-off to Adam run before any launch: no GPU needed."""
import ctypes


def test_backward_without_dirty_word_or_tail_job_is_accepted(hip_lib):
    one = ctypes.c_void_p(16)
    # NULL grad_dirty = "the accumulator may hold anything" (the behaviour before the word existed); an empty batch launches nothing
    assert hip_lib.lae_grid_encode_backward_ex(one, one, one, one, one, 0, 3, 2, 16, 0.5, 16, None, None, 0, 0, 0, 1, 0, 0.0, 1.0,
                                               None, None, None, None, None) == 0
    assert hip_lib.lae_grid_encode_backward_planned(one, one, one, one, 0, 3, 2, 16, 0.5, 16, 0, 0, 0, 1, 0.0, 1.0, None, one,
                                                    None, None, None) == 0
    assert hip_lib.lae_grid_encode_backward_planned(one, one, one, one, 64, 3, 2, 16, 0.5, 16, 0, 0, 0, 1, 0.0, 1.0, None, None,
                                                    None, None, None) == -3          # no plan
    # per-tensor dirty words are optional for the optimizer too
    assert hip_lib.lae_adam_apply_multi(0, None, None, None, None, None, None, None, None, None, None, None, 0.9, 0.99, 1e-15, 0.0,
                                        None) == 0


def field_backward(lib, M=64, L=16, gridtype=0, interp=0, **null):
    one = ctypes.c_void_p(16)
    names = ["grad_sigmas", "grad_rgbs", "enc", "dirs", "h", "rgbs", "sigma_weights", "color_weights", "grad_h", "grad_enc",
             "grad_sigma_weights", "grad_color_weights", "inputs", "offsets", "grad_embeddings"]
    assert set(null) <= set(names)
    a = {n: (None if null.get(n) else one) for n in names}
    return lib.lae_nerf_field_backward(a["grad_sigmas"], a["grad_rgbs"], a["enc"], a["dirs"], a["h"], a["rgbs"], a["sigma_weights"],
                                       a["color_weights"], M, 1.0, a["grad_h"], a["grad_enc"], a["grad_sigma_weights"],
                                       a["grad_color_weights"], 1, None, None, 0, 0, None, None, a["inputs"], a["offsets"],
                                       a["grad_embeddings"], L, 0.5, 16, gridtype, 0, interp, 0.0, 1.0, None, None, None, None, None, None)


def test_field_backward_rejects_bad_arguments_before_any_launch(hip_lib):
    # every pointer either half of the call needs, checked before the first launch (there is no GPU here: a launch would fail
    # with another code)
    for name in ("grad_sigmas", "grad_rgbs", "enc", "dirs", "h", "rgbs", "sigma_weights", "color_weights", "grad_h", "grad_enc",
                 "grad_sigma_weights", "grad_color_weights", "inputs", "offsets", "grad_embeddings"):
        assert field_backward(hip_lib, **{name: True}) == -3, name
    assert field_backward(hip_lib, M=72) == -1              # M % 16
    assert field_backward(hip_lib, gridtype=2) == -1
    assert field_backward(hip_lib, interp=2) == -1
    one = ctypes.c_void_p(16)
    # a deferred loss without its partials
    assert hip_lib.lae_nerf_field_backward(one, one, one, one, one, one, one, one, 64, 1.0, one, one, one, one, 1, None, None, 0, 0, None,
                                           one, one, one, one, 16, 0.5, 16, 0, 0, 0, 0.0, 1.0, None, None, None, None, None, None) == -1
    # a found_inf word needs the host copy of the level sizes (only the binned pipeline can promise it)
    assert hip_lib.lae_nerf_field_backward(one, one, one, one, one, one, one, one, 64, 1.0, one, one, one, one, 1, None, None, 0, 0, None,
                                           None, one, one, one, 16, 0.5, 16, 0, 0, 0, 0.0, 1.0, None, None, one, None, None, None) == -1

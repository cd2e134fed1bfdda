"""The opt-in differentiable facade of the VAE training loop (main_coop_vae.py:452-468), checked before any device work: the default
still refuses gradient callers, `differentiable=True` constructs and passes the guard, and a text tower that is not frozen is refused
(the HIP backward computes the gradient with respect to the prompts only)."""
import inspect

import pytest
import torch

from hoigen_amd import _lib, synth, vae
from hoigen_amd.model import build_model


@pytest.fixture(scope="module")
def model():
    return build_model(synth.to_torch(synth.clip_state_dict(synth.TINY, 10)))


def _call(te, m, grad=True):
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    prompts = torch.zeros(2, 16, m.transformer.width, device=dev, requires_grad=grad)
    tok = torch.zeros(2, 16, dtype=torch.long, device=dev)
    tok[:, 9] = 7
    return te(prompts, tok)


def _reaches_the_device(te, m, grad=True, want_grad_fn=True):
    """the call passed every guard: without a device it fails for the missing device and nothing else; with one it returns the text
    features, attached to the graph exactly when a gradient was asked for"""
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            _call(te, m, grad)
        return
    m.cuda()
    try:
        out = _call(te, m, grad)
        assert out.shape == (2, m.text_projection.shape[1]) and bool(torch.isfinite(out).all())
        assert (out.grad_fn is not None) == want_grad_fn and out.requires_grad == want_grad_fn
    finally:
        m.cpu()


def test_text_encoder_default_still_refuses_and_opt_in_constructs(model):
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match="requires grad"):
            _call(vae.TextEncoder(model).eval(), model)
        with pytest.raises(RuntimeError, match="requires grad"):
            _call(vae.TextEncoder(model, differentiable=False).eval(), model)
        te = vae.TextEncoder(model, differentiable=True).eval()
        assert te.differentiable and not vae.TextEncoder(model).differentiable
        assert list(te.state_dict()) == list(vae.TextEncoder(model).state_dict())      # the same module tree either way


def test_trainable_text_tower_is_refused(model):
    te = vae.TextEncoder(model, differentiable=True).eval()
    with torch.enable_grad():
        model.requires_grad_(True)
        with pytest.raises(RuntimeError, match="frozen text tower"):
            _call(te, model)
        # frozen as main_coop_vae.py:316-318 freezes it: the guard passes and the call reaches the device
        model.requires_grad_(False)
        try:
            _reaches_the_device(te, model)
            # a trainable vision tower is none of this path's business
            model.visual.requires_grad_(True)
            _reaches_the_device(te, model)
        finally:
            model.requires_grad_(True)


def test_differentiable_text_encoder_is_plain_inference_without_a_grad_input(model):
    te = vae.TextEncoder(model, differentiable=True).eval()
    with torch.enable_grad():      # no grad input: the inference call, whatever the tower's flags (its guard still holds in train() mode)
        _reaches_the_device(te, model, grad=False, want_grad_fn=False)
    with torch.no_grad():
        _reaches_the_device(te, model, grad=True, want_grad_fn=False)


def test_prompt_learner_takes_differentiable(model):
    for cls in (vae.PromptLearner_hoi, vae.PromptLearner_h, vae.PromptLearner_o):
        p = inspect.signature(cls.__init__).parameters["differentiable"]
        assert p.default is False
    # building a prompt learner embeds the class names on the device: without one the constructor gets as far as that
    if torch.cuda.is_available():
        pl = vae.PromptLearner_hoi(["ride horse", "hold cup"], model.cuda(), differentiable=True)
        assert pl.differentiable and pl.ctx.requires_grad
        model.cpu()
    else:
        with pytest.raises(RuntimeError, match="HIP device"):
            vae.PromptLearner_hoi(["ride horse", "hold cup"], model, differentiable=True)


def test_bindings_list_the_new_entry_points():
    for name in ("hg_encode_text_embeds_save", "hg_text_backward_embeds", "hg_assemble_prompts_backward", "hg_test_text_grad"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)

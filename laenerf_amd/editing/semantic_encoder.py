"""The semantic encoder of the Ref-NPR second stage (reference: editing/semantic_encoder.py) without torchvision, and the per-view
supervision the stage trains against (editing/single_view_edit_dataset.py:144-161, :267-279).

The VGG-16 feature layers are plain torch modules (MIOpen convolutions: plumbing, as in style_network.py); their weights come from a
file the user already has, in torchvision's `vgg16` state-dict layout (`features.{i}.weight` / `.bias`).  Nothing is downloaded.

    sem = SemanticEncoder(load_vgg16_features("vgg16-397923af.pth", last_layer=29))
    template = extract_ref_template(renderer, pose, intrinsics, H, W, painted, original_rgba)       # ray_registration.py
    sup = build_ref_supervision(views, template, sem, feature_size=256)
    es = RefEditSet.from_views(views, (H, W), supervision=sup)                                      # ref_stage.py

What the reference stores per view and what is kept here:
  * template term: the reference stores `nn_feat_replace(sup_feat, content_feat, style_feat)`, the style features gathered at the
    nearest content position, [3, 256, 64 * 64] fp32 = 12 MB per view.  Here a view keeps the relation z [3, P] int32 (48 KB at
    feature_size 256) and the set the one shared style_feat; the loss `lae_nnfm_loss_forward(x, style_feat, z)` is exactly
    cos_loss(actual_feat, gather(style_feat, z)).
  * colour patch: per position of the relu5 grid the layer (of 25, 27, 29) whose best match is closest decides, the lowest layer on
    ties (torch.argmin), and the position takes the template's mean patch colour at that layer's match.
The matcher (csrc/nnfm.hip) compares fp16 unit vectors with fp32 accumulation: on near ties z (and with it the chosen patch colour)
can differ from an fp32 arg-min; the chosen column's cosine distance stays within the matcher's fp16 margin of the best one
(tests/test_gpu_nnfm.py's criterion).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .style_network import IMAGENET_MEAN, IMAGENET_STD

__all__ = ["VGG16_CFG", "vgg16_features", "load_vgg16_features", "SemanticEncoder", "build_ref_supervision", "TEMPLATE_LAYERS", "COLOR_LAYERS"]

VGG16_CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")
TEMPLATE_LAYERS = (11, 13, 15)          # relu3_1..3: the template feature term
COLOR_LAYERS = (25, 27, 29)             # relu5_1..3: the colour-patch matching


def vgg16_features(last_layer=30):
    """torchvision's vgg16().features[:last_layer + 1] (ReLU not in place), randomly initialised"""
    layers, c_in = [], 3
    for v in VGG16_CFG:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(c_in, v, kernel_size=3, padding=1), nn.ReLU(inplace=False)]
            c_in = v
    if not 0 <= int(last_layer) < len(layers):
        raise ValueError(f"vgg16_features: last_layer must lie in 0..{len(layers) - 1}")
    return nn.Sequential(*layers[:int(last_layer) + 1])


def load_vgg16_features(path_or_state_dict, last_layer):
    """vgg16_features(last_layer) with the conv weights of a torchvision `vgg16` state dict (a path or the dict itself; keys
    `features.{i}.weight` / `.bias`, other keys and layers past last_layer ignored).  Missing keys and wrong shapes raise
    ValueError.  -> nn.Sequential in eval mode, parameters frozen"""
    sd = path_or_state_dict
    if not isinstance(sd, dict):
        sd = torch.load(sd, map_location="cpu", weights_only=True)
    if "state_dict" in sd and isinstance(sd["state_dict"], dict):
        sd = sd["state_dict"]
    net = vgg16_features(last_layer)
    for i, layer in enumerate(net):
        if not isinstance(layer, nn.Conv2d):
            continue
        for name in ("weight", "bias"):
            key = f"features.{i}.{name}"
            if key not in sd:
                raise ValueError(f"load_vgg16_features: missing {key!r}")
            t = torch.as_tensor(sd[key])
            p = getattr(layer, name)
            if tuple(t.shape) != tuple(p.shape):
                raise ValueError(f"load_vgg16_features: {key} has shape {tuple(t.shape)}, VGG-16 needs {tuple(p.shape)}")
            with torch.no_grad():
                p.copy_(t.float())
    for p in net.parameters():
        p.requires_grad_(False)
    return net.eval()


class SemanticEncoder(nn.Module):
    """SemanticEncoder(vgg): `vgg` = load_vgg16_features(...) with at least the layers asked of it (15 for the template term, 29
    for build_ref_supervision).  Parameters are frozen; ReLUs are made out-of-place (features are read before the next layer)."""

    def __init__(self, vgg):
        super().__init__()
        self.backbone = nn.Sequential(*list(vgg))
        for i, layer in enumerate(self.backbone):
            if isinstance(layer, nn.ReLU):
                self.backbone[i] = nn.ReLU(inplace=False)
        for p in self.backbone.parameters():
            p.requires_grad_(False)
        dev = next(self.backbone.parameters()).device
        self.register_buffer("mean", torch.tensor(IMAGENET_MEAN, device=dev).view(3, 1, 1))
        self.register_buffer("std", torch.tensor(IMAGENET_STD, device=dev).view(3, 1, 1))

    def features_from_input(self, x, layers=TEMPLATE_LAYERS):
        """a normalized (and resized) [3,h,w] input -> the outputs of `layers` stacked [L,C,h',w'] (semantic_encoder.py:63-71)"""
        layers = tuple(int(i) for i in layers)
        if not layers or max(layers) >= len(self.backbone):
            raise ValueError(f"SemanticEncoder: the VGG has {len(self.backbone)} layers, layers {layers} asked")
        outs = []
        for i, layer in enumerate(self.backbone):
            if i > max(layers):
                break
            x = layer(x)
            if i in layers:
                outs.append(x)
        if len({tuple(o.shape) for o in outs}) != 1:
            raise ValueError(f"SemanticEncoder: layers {layers} give features of different shapes {[tuple(o.shape) for o in outs]}")
        return torch.stack(outs)

    def encode_feats(self, img, layers=TEMPLATE_LAYERS, size=(256, 256)):
        """semantic_encoder.py:52-73: img [3,h,w] in 0..1 -> normalize, then (size given) torchvision's Resize on a tensor --
        F.interpolate bilinear, align_corners=False, no antialias, the rule of style_network.py -- then the stacked layer outputs"""
        x = (img.float().to(self.mean.device) - self.mean) / self.std
        if size is not None:
            size = (int(size), int(size)) if isinstance(size, int) else tuple(int(s) for s in size)
            x = F.interpolate(x[None], size=size, mode="bilinear", align_corners=False, antialias=False)[0]
        return self.features_from_input(x, layers)

    @staticmethod
    def cos_loss(a, b):
        """semantic_encoder.py:128-135 on [n, C, N] features"""
        a_n = (a * a).sum(1, keepdim=True).sqrt()
        b_n = (b * b).sum(1, keepdim=True).sqrt()
        return (1.0 - ((a / (a_n + 1e-8)) * (b / (b_n + 1e-8))).sum(1)).mean()

    @staticmethod
    def mean_patch_color(img, size):
        """semantic_encoder.py:196-204 (`get_mean_patch_color`): the same Resize of a [3,H,W] image to `size`"""
        return F.interpolate(img.float()[None], size=tuple(int(s) for s in size), mode="bilinear", align_corners=False, antialias=False)[0]


@torch.no_grad()
def build_ref_supervision(views, template, sem, feature_size=256):
    """single_view_edit_dataset.py:144-161 and :267-279, once, eagerly.
    views: the dicts of register_views (cut_gt [h,w,3], `image` [H,W,3|4] the view's training image: its first three channels feed
    the colour features, as the reference's `images[pose_idx, ..., :3]`); template: extract_ref_template's dict -- `painted` [H,W,3]
    (the painted colours on the mask, zero elsewhere), `original` [H,W,3] (the template's training image, first three channels),
    `box` (x_min, x_max, y_min, y_max, exclusive upper bounds as everywhere).
    -> {style_feat [3,C,P] fp32 (the painted crop's features at feature_size, layers 11/13/15), content_feat [3,C,P] (the original
        crop's), patch_mean_color [3,N5] (the painted image resized to the relu5 grid of the original), tmpl_z [V,3,P] int32
        (nnfm_match(view's cut_gt features, content_feat), one problem per layer), color_patch [V,3,ph,pw] fp32, feature_size,
        patch_hw}
    z comes from the fp16 matcher (module docstring): near ties can resolve differently from an fp32 arg-min."""
    from .nnfm import nnfm_match, nnfm_pack
    dev = sem.mean.device
    S = int(feature_size)
    x0, x1, y0, y1 = (int(v) for v in template["box"])
    painted = torch.as_tensor(template["painted"]).to(dev).float()[..., :3]
    original = torch.as_tensor(template["original"]).to(dev).float()[..., :3]
    if x1 - x0 < 1 or y1 - y0 < 1:
        raise ValueError("build_ref_supervision: the template's crop box is empty")
    style_feat = sem.encode_feats(painted[x0:x1, y0:y1].permute(2, 0, 1), TEMPLATE_LAYERS, (S, S)).flatten(2).float().contiguous()
    content_feat = sem.encode_feats(original[x0:x1, y0:y1].permute(2, 0, 1), TEMPLATE_LAYERS, (S, S)).flatten(2).float().contiguous()
    color_feat = sem.encode_feats(original.permute(2, 0, 1), COLOR_LAYERS, None)
    ph, pw = int(color_feat.shape[-2]), int(color_feat.shape[-1])
    color_feat = color_feat.flatten(2).float().contiguous()
    patch_mean = sem.mean_patch_color(painted.permute(2, 0, 1), (ph, pw)).flatten(1).contiguous()              # [3, ph*pw]
    packed_content, packed_color = nnfm_pack(content_feat), nnfm_pack(color_feat)
    zs, patches = [], []
    for k, v in enumerate(views):
        if "image" not in v:
            raise ValueError(f"build_ref_supervision: view {k} has no 'image' (its training image, [H,W,3|4])")
        sup = sem.encode_feats(torch.as_tensor(v["cut_gt"]).to(dev).permute(2, 0, 1), TEMPLATE_LAYERS, (S, S)).flatten(2).float().contiguous()
        zs.append(nnfm_match(sup, content_feat, packed_b=packed_content))
        img = torch.as_tensor(v["image"]).to(dev).float()[..., :3]
        col = sem.encode_feats(img.permute(2, 0, 1), COLOR_LAYERS, None)
        if tuple(col.shape[-2:]) != (ph, pw):
            raise ValueError(f"build_ref_supervision: view {k}'s image gives a {tuple(col.shape[-2:])} relu5 grid, the template's {(ph, pw)}")
        z, dist = nnfm_match(col.flatten(2).float().contiguous(), color_feat, return_distance=True, packed_b=packed_color)
        best = dist.argmin(0)                                              # the closest layer per position, the lowest on ties
        zc = z.gather(0, best[None]).long()[0]
        patches.append(patch_mean[:, zc].reshape(3, ph, pw))
    return {"style_feat": style_feat, "content_feat": content_feat, "patch_mean_color": patch_mean, "tmpl_z": torch.stack(zs).to(torch.int32),
            "color_patch": torch.stack(patches).float(), "feature_size": S, "patch_hw": (ph, pw)}

"""The VGG style network of LAENeRF's stylization (reference: editing/style_network.py) without torchvision.

The VGG-19 feature layers are plain torch modules (MIOpen convolutions: plumbing, not a hand-written hot path); their weights come
from a file the user already has, in torchvision's `vgg19` state-dict layout (`features.{i}.weight` / `.bias`, e.g.
vgg19-dcbb9e9d.pth).  Nothing is downloaded.

    vgg = load_vgg19_features("vgg19-dcbb9e9d.pth", last_layer=14)
    net = StyleNetwork(load_style_image("style.png"), vgg)          # gram_style from a RandomCrop of the style image
    loss = net(img)                                                  # img [3,h,w]: resize -> normalize -> VGG -> Gram -> MSE

What the reference does and this restates (editing/style_network.py:63-191):
  * the style features are the outputs of the layers `style_layers` (default (10, 12, 14): conv outputs before their ReLU) of
    vgg19.features[:max + 1] with ReLU(inplace=False), run on an UNBATCHED [3,S,S] tensor and stacked into [L,C,h,w];
  * gram = F F^T / (C h w) per layer; the loss is the MSE between the Gram stacks;
  * gram_style comes from torchvision's RandomCrop(S, pad_if_needed=True) of the style image: a short side is padded on BOTH sides by
    its deficit, then the crop starts at torch.randint offsets (`crop_offset` fixes them, `generator` draws them);
  * `match_color` (preserve_color): the view's target colours are matched to the style image through 3x3 covariance square roots,
    and the Gram of the un-normalized, full-resolution matched image becomes the target.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

__all__ = ["VGG19_CFG", "vgg19_features", "load_vgg19_features", "load_style_image", "random_crop_params", "random_crop", "gram_matrix",
           "StyleNetwork", "IMAGENET_MEAN", "IMAGENET_STD"]

VGG19_CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512, "M")
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def vgg19_features(last_layer=36):
    """torchvision's vgg19().features[:last_layer + 1] (ReLU not in place), randomly initialised"""
    layers, c_in = [], 3
    for v in VGG19_CFG:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(c_in, v, kernel_size=3, padding=1), nn.ReLU(inplace=False)]
            c_in = v
    if not 0 <= int(last_layer) < len(layers):
        raise ValueError(f"vgg19_features: last_layer must lie in 0..{len(layers) - 1}")
    return nn.Sequential(*layers[:int(last_layer) + 1])


def load_vgg19_features(path_or_state_dict, last_layer):
    """vgg19_features(last_layer) with the conv weights of a torchvision `vgg19` state dict (a path or the dict itself; keys
    `features.{i}.weight` / `.bias`, other keys and layers past last_layer ignored).  Missing keys, keys of layers that have no
    weights and wrong shapes raise ValueError.  -> nn.Sequential in eval mode, parameters frozen"""
    sd = path_or_state_dict
    if not isinstance(sd, dict):
        sd = torch.load(sd, map_location="cpu", weights_only=True)
    if "state_dict" in sd and isinstance(sd["state_dict"], dict):
        sd = sd["state_dict"]
    net = vgg19_features(last_layer)
    n = len(net)
    for k in sd:
        parts = k.split(".")
        if len(parts) == 3 and parts[0] == "features" and parts[1].isdigit() and int(parts[1]) < n:
            if not isinstance(net[int(parts[1])], nn.Conv2d) or parts[2] not in ("weight", "bias"):
                raise ValueError(f"load_vgg19_features: unexpected key {k!r} (layer {parts[1]} is {type(net[int(parts[1])]).__name__})")
    for i, layer in enumerate(net):
        if not isinstance(layer, nn.Conv2d):
            continue
        for name in ("weight", "bias"):
            key = f"features.{i}.{name}"
            if key not in sd:
                raise ValueError(f"load_vgg19_features: missing {key!r}")
            t = torch.as_tensor(sd[key])
            p = getattr(layer, name)
            if tuple(t.shape) != tuple(p.shape):
                raise ValueError(f"load_vgg19_features: {key} has shape {tuple(t.shape)}, VGG-19 needs {tuple(p.shape)}")
            with torch.no_grad():
                p.copy_(t.float())
    for p in net.parameters():
        p.requires_grad_(False)
    return net.eval()


def load_style_image(path):
    """the style image as [3,H,W] fp32 in [0,1] (PIL decode, converted to RGB; the reference reads it with torchvision.io / 255)"""
    import numpy as np
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im.convert("RGB"), dtype=np.uint8)
    return torch.from_numpy(a.copy()).permute(2, 0, 1).float() / 255.0


def random_crop_params(height, width, size, generator=None):
    """torchvision 0.15.2 RandomCrop(size, pad_if_needed=True) on an image of height x width: -> (pad_w, pad_h, i, j).  A side
    shorter than size is padded by its deficit on BOTH ends (F.pad with [deficit, 0] / [0, deficit]); then i, j =
    torch.randint(0, H' - size + 1), torch.randint(0, W' - size + 1), or (0, 0) when the padded image is exactly size x size"""
    pad_w = size - width if width < size else 0
    pad_h = size - height if height < size else 0
    H, W = height + 2 * pad_h, width + 2 * pad_w
    if H == size and W == size:
        return pad_w, pad_h, 0, 0
    i = int(torch.randint(0, H - size + 1, size=(1,), generator=generator).item())
    j = int(torch.randint(0, W - size + 1, size=(1,), generator=generator).item())
    return pad_w, pad_h, i, j


def random_crop(img, size, generator=None, crop_offset=None):
    """img [C,H,W] -> [C,size,size] by the rule of random_crop_params (crop_offset = (i, j) replaces the draw)"""
    _, h, w = img.shape
    pad_w, pad_h, i, j = random_crop_params(h, w, size, generator) if crop_offset is None else \
        (size - w if w < size else 0, size - h if h < size else 0, int(crop_offset[0]), int(crop_offset[1]))
    if pad_w or pad_h:
        img = F.pad(img, (pad_w, pad_w, pad_h, pad_h))
    if not (0 <= i <= img.shape[1] - size and 0 <= j <= img.shape[2] - size):
        raise ValueError("random_crop: the crop offset leaves the padded image")
    return img[:, i:i + size, j:j + size]


def gram_matrix(feats):
    """[L,C,h,w] -> [L,C,C]: F F^T / (C h w) per layer (fp32 matmul)"""
    L, C, h, w = feats.shape
    f = feats.reshape(L, C, h * w)
    return torch.bmm(f, f.transpose(1, 2)) / (C * h * w)


class StyleNetwork(nn.Module):
    """StyleNetwork(style_image [3,H,W], vgg, style_layers=(10, 12, 14), size=256, crop_offset=None, generator=None, loss="gram",
    nnfm_match="concat").
    `vgg`: load_vgg19_features(...) (at least max(style_layers) + 1 layers).  Buffers: gram_style (of the random crop) and gram_target
    (what the loss compares against: gram_style, or the colour-matched Gram after match_color).
    The chosen loss is kept as `loss_kind`.  loss="nnfm": loss_from_input is the nearest-neighbour feature matching loss
    (editing/nnfm.py) against the crop's features;
    further buffers nnfm_style [L,C,h'w'] (the crop's features), nnfm_target (what the loss matches against) and nnfm_packed (the
    matcher's fp16 copy of nnfm_target in the `nnfm_match` arrangement: "concat" = the layers concatenated, one matching; "layer" =
    one matching per layer).  match_color then also re-derives the NNFM target: the features of the SAME crop of the matched
    image, normalized as at construction, so the buffers keep their shapes and addresses (captured steps read them)."""

    def __init__(self, style_image, vgg, style_layers=(10, 12, 14), size=256, crop_offset=None, generator=None, loss="gram",
                 nnfm_match="concat"):
        super().__init__()
        if loss not in ("gram", "nnfm"):
            raise ValueError(f"StyleNetwork: loss must be 'gram' or 'nnfm', not {loss!r}")
        if nnfm_match not in ("concat", "layer"):
            raise ValueError(f"StyleNetwork: nnfm_match must be 'concat' or 'layer', not {nnfm_match!r}")
        self.loss_kind, self.nnfm_match = loss, nnfm_match
        self.style_layers = tuple(int(i) for i in style_layers)
        if not self.style_layers:
            raise ValueError("StyleNetwork: no style layers")
        if max(self.style_layers) >= len(vgg):
            raise ValueError(f"StyleNetwork: the VGG has {len(vgg)} layers, style layer {max(self.style_layers)} is missing")
        self.vgg = nn.Sequential(*list(vgg)[:max(self.style_layers) + 1])
        for i, layer in enumerate(self.vgg):
            if isinstance(layer, nn.ReLU):
                self.vgg[i] = nn.ReLU(inplace=False)
        for p in self.vgg.parameters():
            p.requires_grad_(False)
        self.size = int(size)
        dev = next(self.vgg.parameters()).device
        img = style_image.detach().float().to(dev)
        if img.dim() != 3 or img.shape[0] != 3:
            raise ValueError("StyleNetwork: the style image must be [3,H,W]")
        self.register_buffer("image", img)
        self.register_buffer("mean", torch.tensor(IMAGENET_MEAN, device=dev).view(3, 1, 1))
        self.register_buffer("std", torch.tensor(IMAGENET_STD, device=dev).view(3, 1, 1))
        with torch.no_grad():
            if crop_offset is None:                    # the draw random_crop would make, kept for match_color's NNFM target
                crop_offset = random_crop_params(img.shape[1], img.shape[2], self.size, generator)[2:]
            self.crop_offset = (int(crop_offset[0]), int(crop_offset[1]))
            crop = random_crop(img, self.size, crop_offset=self.crop_offset)
            feats = self.features(self.normalize(crop))
            gs = gram_matrix(feats)
        self.register_buffer("gram_style", gs)
        self.register_buffer("gram_target", gs.clone())
        if loss == "nnfm":
            from .nnfm import nnfm_pack, _as_problems
            fs = feats.flatten(2).float().contiguous()
            self.register_buffer("nnfm_style", fs)
            self.register_buffer("nnfm_target", fs.clone())
            self.register_buffer("nnfm_packed", nnfm_pack(_as_problems(fs, nnfm_match)))

    def normalize(self, img):
        return (img - self.mean) / self.std

    def resize(self, img):
        """torchvision Resize((S, S)) on a [3,h,w] tensor: bilinear, align_corners=False, no antialias"""
        return F.interpolate(img[None], size=(self.size, self.size), mode="bilinear", align_corners=False, antialias=False)[0]

    def features(self, x):
        """[3,h,w] -> the style layers' outputs stacked [L,C,h',w'] (shapes must agree, as the reference's stack requires)"""
        outs = []
        for i, layer in enumerate(self.vgg):
            x = layer(x)
            if i in self.style_layers:
                outs.append(x)
        if len({tuple(o.shape) for o in outs}) != 1:
            raise ValueError(f"StyleNetwork: the style layers {self.style_layers} give features of different shapes "
                             f"{[tuple(o.shape) for o in outs]}")
        return torch.stack(outs)

    def loss_from_input(self, vgg_in):
        """the style loss of the normalized [3,S,S] VGG input: MSE(gram(vgg(vgg_in)), gram_target), or with loss="nnfm" the
        nearest-neighbour feature matching loss of vgg(vgg_in) against nnfm_target"""
        if self.loss_kind == "nnfm":
            from .nnfm import nnfm_loss
            return nnfm_loss(self.features(vgg_in), self.nnfm_target, packed_style=self.nnfm_packed, match=self.nnfm_match)
        return F.mse_loss(gram_matrix(self.features(vgg_in)), self.gram_target)

    def forward(self, img):
        """the reference's forward (style_network.py:183-191): img [3,h,w] -> resize -> normalize -> VGG -> Gram -> MSE"""
        return self.loss_from_input(self.normalize(self.resize(img)))

    @torch.no_grad()
    def match_color(self, target_img, eps=1e-5):
        """style_network.py:93-123: the style image re-coloured to the statistics of target_img ([3,K] or [3,h,w]); the Gram of the
        matched image (un-normalized, full resolution, as the reference computes it) becomes gram_target.  -> the matched image"""
        img = self.image
        mu_t = img.mean(dim=(1, 2), keepdim=True)
        t = (img - mu_t).flatten(1, 2)
        Ct = t @ t.T / t.shape[1] + eps * torch.eye(3, device=t.device)
        target_img = target_img.float().to(img.device)
        if target_img.dim() == 2:
            target_img = target_img[..., None]
        mu_s = target_img.mean(dim=(1, 2), keepdim=True)
        s = (target_img - mu_s).flatten(1, 2)
        Cs = s @ s.T / s.shape[1] + eps * torch.eye(3, device=s.device)
        eva_t, eve_t = torch.linalg.eigh(Ct)
        Qt = eve_t @ torch.sqrt(torch.diag(eva_t)) @ eve_t.T
        eva_s, eve_s = torch.linalg.eigh(Cs)
        Qs = eve_s @ torch.sqrt(torch.diag(eva_s)) @ eve_s.T
        ts = Qs @ torch.linalg.inv(Qt) @ t
        matched = torch.clamp(ts.reshape(img.shape) + mu_s, 0, 1)
        self.gram_target.copy_(gram_matrix(self.features(matched)))
        if self.loss_kind == "nnfm":
            crop = random_crop(matched, self.size, crop_offset=self.crop_offset)
            self._set_nnfm_target(self.features(self.normalize(crop)).flatten(2).float())
        return matched

    def _set_nnfm_target(self, feats):
        """nnfm_target and its packed copy, in place"""
        from ..backend import nnfm_backend
        from .nnfm import _as_problems
        self.nnfm_target.copy_(feats)
        f = _as_problems(self.nnfm_target, self.nnfm_match)
        nnfm_backend.pack(f, f.shape[0], f.shape[1], f.shape[2], self.nnfm_packed)

    def reset_target(self):
        """gram_target = gram_style (and the NNFM target = the crop's features)"""
        with torch.no_grad():
            self.gram_target.copy_(self.gram_style)
            if self.loss_kind == "nnfm":
                self._set_nnfm_target(self.nnfm_style)

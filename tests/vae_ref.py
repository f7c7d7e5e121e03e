"""Float64 functional restatement of the SDS guidance's differentiable chain, written from DESIGN.md 9f with F.interpolate /
F.conv2d / F.group_norm / F.silu / softmax: the Stable-Diffusion-2.1 VAE encoder (ldm ``Encoder`` + ``quant_conv``, ldm key layout)
with the resize and ``x * 2 - 1`` in front, the posterior sample, and ImageDream's loss tail (imagedream_guidance.py:225-352) -- the
oracle of tests/test_sds_*.py.  ``ch`` is a parameter so that the CPU tests can gradcheck a narrow copy."""
import torch
import torch.nn.functional as F

CH_MULT = (1, 2, 4, 4)
Z = 4
SCALE_FACTOR = 0.18215


def _block_keys(p, cin, cout):
    out = [(f"{p}.norm1.weight", (cin,)), (f"{p}.norm1.bias", (cin,)), (f"{p}.conv1.weight", (cout, cin, 3, 3)), (f"{p}.conv1.bias", (cout,)),
           (f"{p}.norm2.weight", (cout,)), (f"{p}.norm2.bias", (cout,)), (f"{p}.conv2.weight", (cout, cout, 3, 3)), (f"{p}.conv2.bias", (cout,))]
    if cin != cout:
        out += [(f"{p}.nin_shortcut.weight", (cout, cin, 1, 1)), (f"{p}.nin_shortcut.bias", (cout,))]
    return out


def keys(ch=128):
    """(ldm key, shape) of the encoder and quant_conv at width ch"""
    out = [("encoder.conv_in.weight", (ch, 3, 3, 3)), ("encoder.conv_in.bias", (ch,))]
    c = ch
    for i, m in enumerate(CH_MULT):
        for j in range(2):
            out += _block_keys(f"encoder.down.{i}.block.{j}", c, ch * m)
            c = ch * m
        if i < 3:
            out += [(f"encoder.down.{i}.downsample.conv.weight", (c, c, 3, 3)), (f"encoder.down.{i}.downsample.conv.bias", (c,))]
    out += _block_keys("encoder.mid.block_1", c, c)
    out += [("encoder.mid.attn_1.norm.weight", (c,)), ("encoder.mid.attn_1.norm.bias", (c,))]
    for n in ("q", "k", "v", "proj_out"):
        out += [(f"encoder.mid.attn_1.{n}.weight", (c, c, 1, 1)), (f"encoder.mid.attn_1.{n}.bias", (c,))]
    out += _block_keys("encoder.mid.block_2", c, c)
    out += [("encoder.norm_out.weight", (c,)), ("encoder.norm_out.bias", (c,)), ("encoder.conv_out.weight", (2 * Z, c, 3, 3)),
            ("encoder.conv_out.bias", (2 * Z,)), ("quant_conv.weight", (2 * Z, 2 * Z, 1, 1)), ("quant_conv.bias", (2 * Z,))]
    return out


def random_weights(seed=0, ch=128, attn_gain=1.0):
    """Seeded ldm-layout weights (float32, CPU), scaled so that activations stay O(1) through all 32 convolutions: fan-in scaled
    convolutions (the second of a block and proj_out at half that, so the residual stream grows slowly), GroupNorm affines near
    (1, 0), attention scores O(1).  attn_gain multiplies the attention's q and k weights (the scores by its square): at 1 the
    softmax is close to uniform, at 2 - 3 a row has a dominant key (``attention_probs`` measures it); the other tensors do not
    depend on it."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in keys(ch):
        if k.endswith(".bias"):
            sd[k] = torch.randn(shape, generator=g) * 0.05
        elif "norm" in k:                       # GroupNorm weight
            sd[k] = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            fan_in = shape[1] * shape[2] * shape[3]
            scale = 0.5 if (".conv2." in k or "proj_out" in k) else 1.0
            sd[k] = torch.randn(shape, generator=g) * (scale / fan_in ** 0.5)
    if attn_gain != 1.0:
        for n in ("q", "k"):
            sd[f"encoder.mid.attn_1.{n}.weight"] = sd[f"encoder.mid.attn_1.{n}.weight"] * attn_gain
    return sd


def cast(sd, dtype, device=None, prefix=""):
    return {k[len(prefix):] if k.startswith(prefix) else k: v.to(device=device, dtype=dtype) for k, v in sd.items()}


def _gn(x, w, p, silu=True):
    h = F.group_norm(x, 32, w[p + ".weight"], w[p + ".bias"], eps=1e-6)
    return F.silu(h) if silu else h


def _conv(x, w, p, **kw):
    return F.conv2d(x, w[p + ".weight"], w[p + ".bias"], **kw)


def _resblock(x, w, p):
    h = _conv(_gn(x, w, p + ".norm1"), w, p + ".conv1", padding=1)
    h = _conv(_gn(h, w, p + ".norm2"), w, p + ".conv2", padding=1)
    if p + ".nin_shortcut.weight" in w:
        x = _conv(x, w, p + ".nin_shortcut")
    return x + h


def _attn_probs(h, w, p):
    """the normed input [B, C, H, W] -> softmax(q^T k / sqrt(C)) [B, T, T] (rows: queries) and v"""
    q, k, v = (_conv(h, w, f"{p}.{n}") for n in ("q", "k", "v"))
    B, C, H, W = q.shape
    q = q.reshape(B, C, H * W).permute(0, 2, 1)
    k = k.reshape(B, C, H * W)
    s = torch.bmm(q, k) * (int(C) ** (-0.5))
    return torch.softmax(s, dim=2), v


def _attn(x, w, p):
    h = _gn(x, w, p + ".norm", silu=False)
    s, v = _attn_probs(h, w, p)
    B, C, H, W = v.shape
    v = v.reshape(B, C, H * W)
    o = torch.bmm(v, s.permute(0, 2, 1)).reshape(B, C, H, W)
    return x + _conv(o, w, p + ".proj_out")


def _to_mid(x, w, image_size):
    """the resize, conv_in, the four levels and mid.block_1: the attention block's input"""
    x = F.interpolate(x, (image_size, image_size), mode="bilinear", align_corners=False) * 2 - 1
    h = _conv(x, w, "encoder.conv_in", padding=1)
    for i in range(4):
        for j in range(2):
            h = _resblock(h, w, f"encoder.down.{i}.block.{j}")
        if i < 3:
            h = _conv(F.pad(h, (0, 1, 0, 1)), w, f"encoder.down.{i}.downsample.conv", stride=2)
    return _resblock(h, w, "encoder.mid.block_1")


def attention_probs(x, w, image_size):
    """x [N, 3, H, W] -> the attention's softmax matrix [N, T, T], T = (image_size / 8)^2, row = query"""
    h = _gn(_to_mid(x, w, image_size), w, "encoder.mid.attn_1.norm", silu=False)
    return _attn_probs(h, w, "encoder.mid.attn_1")[0]


def moments(x, w, image_size):
    """x [N, 3, H, W] in [0, 1] -> (mean, logvar) [N, 4, s/8, s/8], logvar clamped"""
    h = _to_mid(x, w, image_size)
    h = _attn(h, w, "encoder.mid.attn_1")
    h = _resblock(h, w, "encoder.mid.block_2")
    h = _conv(_gn(h, w, "encoder.norm_out"), w, "encoder.conv_out", padding=1)
    m = _conv(h, w, "quant_conv")
    mean, logvar = torch.chunk(m, 2, dim=1)
    return mean, torch.clamp(logvar, -30.0, 20.0)


def latents(x, w, image_size, eps, scale_factor=SCALE_FACTOR):
    mean, logvar = moments(x, w, image_size)
    return scale_factor * (mean + torch.exp(0.5 * logvar) * eps)


# ---- the loss tail ----
def ldm_alphas_cumprod(n=1000, start=0.00085, end=0.012):
    betas = torch.linspace(start ** 0.5, end ** 0.5, n, dtype=torch.float64) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def tables(ac):
    """ldm's buffers, computed in float64 and stored as float32 (as register_schedule's to_torch does)"""
    ac = ac.to(torch.float64)
    return {"sqrt_ac": ac.sqrt().float(), "sqrt_1m_ac": (1 - ac).sqrt().float(), "sqrt_recip_ac": (1 / ac).sqrt().float(),
            "sqrt_recipm1_ac": (1 / ac - 1).sqrt().float(), "ac": ac.float()}


def q_sample(lat, t, noise, tb):
    return tb["sqrt_ac"][t].to(lat) * lat + tb["sqrt_1m_ac"][t].to(lat) * noise


def loss_tail(lat, noise, eps_pred, t, tb, guidance_scale, n_view, recon_loss=True, recon_std_rescale=0.2, grad_clip=None):
    """imagedream_guidance.py:225-352 after the UNet, lat requiring grad -> (loss, grad_norm, d loss / d lat)"""
    lat = lat.detach().requires_grad_(True)
    x_t = q_sample(lat.detach(), t, noise, tb)
    e_text, e_uncond = eps_pred.chunk(2)
    e = e_uncond + guidance_scale * (e_text - e_uncond)
    if recon_loss:
        sr, srm = tb["sqrt_recip_ac"][t].to(lat), tb["sqrt_recipm1_ac"][t].to(lat)
        recon = sr * x_t - srm * e
        if recon_std_rescale > 0:
            nocfg = sr * x_t - srm * e_text
            nr = nocfg.view(-1, n_view, *nocfg.shape[1:])
            rr = recon.view(-1, n_view, *recon.shape[1:])
            factor = (nr.std([1, 2, 3, 4], keepdim=True) + 1e-8) / (rr.std([1, 2, 3, 4], keepdim=True) + 1e-8)
            adjust = recon.clone() * factor.squeeze(1).repeat_interleave(n_view, dim=0)
            recon = recon_std_rescale * adjust + (1 - recon_std_rescale) * recon
        loss = 0.5 * F.mse_loss(lat, recon.detach(), reduction="sum") / lat.shape[0]
        grad = torch.autograd.grad(loss, lat, retain_graph=True)[0]
    else:
        wt = 1 - tb["ac"][t].to(lat)
        grad = wt * (e - noise)
        if grad_clip is not None:
            grad = grad.clamp(-grad_clip, grad_clip)
        grad = torch.nan_to_num(grad)
        target = (lat - grad).detach()
        loss = 0.5 * F.mse_loss(lat, target, reduction="sum") / lat.shape[0]
    (dlat,) = torch.autograd.grad(loss, lat)
    return loss.detach(), grad.norm().detach(), dlat


def images(N, H, W, seed):
    """renderer-like inputs in [0, 1]: a smooth random image inside an ellipse over a constant background"""
    g = torch.Generator().manual_seed(seed)
    lo = torch.rand(N, 3, max(2, H // 16), max(2, W // 16), generator=g)
    x = F.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    mask = ((yy / 0.8) ** 2 + (xx / 0.6) ** 2 < 1).to(torch.float32)
    return x * mask + 0.5 * (1 - mask)

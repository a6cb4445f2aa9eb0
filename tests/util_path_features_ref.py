"""The reference of decode_ops.path_features_autograd: the torch lines of S2SDAGFastSpeech2Loss's argmax branch (criterions.py, copied as
they stand — clone, path[:, 0] = -1, mask, sum, stable argsort of an int8 tensor, the host read of the widest count, lengths-to-mask, gather
through an expanded index, masked_fill), brought to a given width by a slice or by zero / True padding; a plain Python loop over the vertices
that tests/test_path_features_ref.py holds them to, bit for bit; and the planted paths of the tests.  Pure torch: tensors of any device."""
import torch
import torch.nn.functional as F

PLANTED = ("only_vertex_0", "vertices_63_64", "last_vertex", "every_vertex", "all_fives")


def _lengths_to_mask(lens, n):
    return torch.arange(n, device=lens.device).unsqueeze(0) < lens.unsqueeze(1)


def torch_lines(features, path, skip_first=True):
    """(features_on_path, features_padding_mask, n_on) as the criterion's lines give them, the width the widest count; skip_first=False
    leaves the `path[:, 0] = -1` line out"""
    with torch.no_grad():
        path = path.clone()
        if skip_first:
            path[:, 0] = -1                                                                                  # mask <bos>
        features_mask = path >= 0
        n_on = features_mask.sum(-1)
        order = torch.argsort((~features_mask).to(torch.int8), dim=1, stable=True)[:, : int(n_on.max())]
        features_padding_mask = ~_lengths_to_mask(n_on, order.shape[1])
    features_on_path = features.gather(1, order.unsqueeze(-1).expand(-1, -1, features.shape[-1])) \
        .masked_fill(features_padding_mask.unsqueeze(-1), 0)
    return features_on_path, features_padding_mask, n_on


def reference(features, path, width, skip_first=True):
    """the torch lines at width `width`: the surplus columns sliced off, or zero rows / True / unchanged counts appended; n = min(n_on, width)"""
    out, pad, n_on = torch_lines(features, path, skip_first)
    have = out.shape[1]
    if width < have:
        out, pad = out[:, :width], pad[:, :width]
    elif width > have:
        out = F.pad(out, (0, 0, 0, width - have))
        pad = F.pad(pad, (0, width - have), value=True)
    return out, pad, n_on.clamp(max=width)


def backward_of(fn, features, path, width, dy, skip_first=True):
    """(out, pad, n, dfeatures) of fn(features, path, width, skip_first) with the gradient dy [B, width, C] sent into out"""
    x = features.detach().requires_grad_(True)
    out, pad, n = fn(x, path, width, skip_first)
    out.backward(dy)
    return out.detach(), pad, n, x.grad


def loop(features, path, width, dy=None, skip_first=True):
    """the definition, vertex by vertex on the host: (out, pad, n, dfeatures or None)"""
    B, L, C = features.shape
    out = torch.zeros((B, width, C), dtype=features.dtype)
    pad = torch.ones((B, width), dtype=torch.bool)
    n = torch.zeros((B,), dtype=torch.int64)
    dx = None if dy is None else torch.zeros((B, L, C), dtype=features.dtype)
    for b in range(B):
        r = 0
        for j in range(L):
            if int(path[b, j]) >= 0 and (j > 0 or not skip_first):
                if r < width:
                    out[b, r] = features[b, j]
                    pad[b, r] = False
                    if dx is not None:
                        dx[b, j] = dy[b, r]
                r += 1
        n[b] = min(r, width)
    return out, pad, n, dx


def ranks_where(on):
    """a path in the form the alignment gives it: the rank (0, 1, 2, ...) where `on` is set, -1 elsewhere; int64"""
    on = on.to(torch.bool)
    return torch.where(on, on.to(torch.int64).cumsum(1) - 1, torch.full_like(on, -1, dtype=torch.int64))


def random_path(B, L, seed, fractions=(0.6, 0.0, 0.25)):
    """sample b has about fractions[b % 3] of its vertices on the path (0.0: not one, vertex 0 included), vertex 0 on wherever any is"""
    g = torch.Generator().manual_seed(seed)
    on = torch.stack([torch.rand(L, generator=g) < fractions[b % len(fractions)] for b in range(B)])
    on[:, 0] = on.any(1)
    return ranks_where(on)


def planted_path(name, B, L):
    on = torch.zeros((B, L), dtype=torch.bool)
    if name == "only_vertex_0":                                  # the count is 0 with skip_first
        on[:, 0] = True
    elif name == "vertices_63_64":                               # the last lane of one chunk and the first of the next
        on[:, 0] = True
        on[:, 63:65] = True
    elif name == "last_vertex":
        on[:, 0] = True
        on[:, L - 1] = True
    elif name == "every_vertex":
        on[:] = True
    elif name == "all_fives":                                    # values that are no ranks: only the sign counts
        return torch.where(random_path(B, L, 5) >= 0, 5, -1)
    else:
        raise ValueError(name)
    return ranks_where(on)


def make_features(B, L, C, dtype, seed, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((B, L, C), generator=g).to(dtype).to(device)

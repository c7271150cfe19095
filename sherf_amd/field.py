"""Geometry extraction on top of the field query (ImportanceRenderer.query_points / TriPlaneGenerator.sample): a density grid for marching cubes,
cross-sections or occupancy checks.  Mesh extraction itself is left to the caller."""
import torch

SHELL = 0.05          # the 5 cm shell outside which the field is empty (renderer.py:318)


def default_bounds(input_data):
    """[2, 3] (min, max): the posed vertices' box grown by the 5 cm shell -- everything outside has sigma -80."""
    v = input_data['vertices'].detach().float().reshape(-1, 3)
    return torch.stack([v.min(0)[0] - SHELL, v.max(0)[0] + SHELL])


def grid_centres(bounds, resolution):
    """Voxel centres of a D x H x W grid over `bounds` [2, 3] = (min, max) in (x, y, z): axis 0 of the grid runs along z, axis 1 along y, axis 2 along x
    (a [D, H, W] volume as marching cubes takes it).  -> [D, H, W, 3] fp32 world-frame points (x, y, z)."""
    D, H, W = (resolution,) * 3 if isinstance(resolution, int) else tuple(int(r) for r in resolution)
    b = bounds.detach().float()
    ax = [b[0, a] + (torch.arange(n, device=b.device, dtype=torch.float32) + 0.5) * ((b[1, a] - b[0, a]) / n) for a, n in ((0, W), (1, H), (2, D))]
    z, y, x = torch.meshgrid(ax[2], ax[1], ax[0], indexing='ij')
    return torch.stack([x, y, z], -1)


def density_grid(G, ws_or_z, c, input_data, resolution, bounds=None, direction=(0, 0, -1)):
    """sigma and rgb of generator `G`'s field at the voxel centres of a grid over `bounds` (default: `default_bounds`).
    ws_or_z: latent codes `ws` [1, num_ws, w_dim] (-> G.sample_mixed) or `z` (2-D, or None: SHERF's mapping takes its code from the observation image;
    -> G.sample with `c`).  resolution: an int or (D, H, W).  direction: the view direction every point is queried with (rgb depends on it, sigma does not).
    -> (sigma [D, H, W] raw densities, -80 outside the shell; rgb [D, H, W, 3]; mask [D, H, W] bool; bounds [2, 3])."""
    dev = input_data['vertices'].device
    bounds = default_bounds(input_data) if bounds is None else torch.as_tensor(bounds, dtype=torch.float32, device=dev).reshape(2, 3)
    pts = grid_centres(bounds, resolution)
    D, H, W = pts.shape[:3]
    pts = pts.reshape(1, -1, 3).contiguous()
    dirs = torch.as_tensor(direction, dtype=torch.float32, device=dev).reshape(1, 1, 3).expand(1, pts.shape[1], 3).contiguous()
    with torch.no_grad():
        if torch.is_tensor(ws_or_z) and ws_or_z.ndim == 3:
            out = G.sample_mixed(pts, dirs, ws_or_z, input_data=input_data)
        else:
            out = G.sample(pts, dirs, ws_or_z, c, input_data=input_data)
    return out['sigma'].reshape(D, H, W), out['rgb'].reshape(D, H, W, 3), out['mask'].reshape(D, H, W), bounds

"""Torch front end of the device renderer (include/minigrid_render.h): MiniGridEnv.get_full_render and get_pov_render
of the reference (gym_minigrid/minigrid.py:662-747, 1498-1563 and rendering.py) for N worlds kept as
structure-of-arrays planes on the GPU, byte for byte.  A tile atlas is rasterised once per (device, tile size); a frame
is then a gather from it.  agent_* are 1-D int32 device tensors, dense or the column views of the engine's records
(TwoarmyEngine.agent_views()); their shared stride is what the C ABI is told.  No CPU fallback."""
import torch

from . import _lib
from ._marshal import agent_arrays, call, ptr

MG_RENDER_TILES = 600
MG_RENDER_MAX_TILE = 256


def atlas_bytes(tile_size):
    """Bytes of the atlas of one tile size (host only)."""
    n = _lib.lib().mg_render_atlas_bytes(int(tile_size))
    if n < 0:
        raise ValueError("tile_size must be 1..%d" % MG_RENDER_MAX_TILE)
    return n


def tile_index(type_idx, colour_idx, state=0, agent_dir=-1, highlight=False):
    """Atlas slot of a cell, -1 if the renderer does not draw it (host only)."""
    return _lib.lib().mg_render_tile_index(int(type_idx), int(colour_idx), int(state), int(agent_dir), int(bool(highlight)))


class TileAtlas:
    """Every drawable tile (object x colour x door state x agent direction x highlight) at one tile size:
    `tiles` uint8[600, ts, ts, 3] on the device.  TileAtlas.get() builds one per (device, tile size) and keeps it."""
    _cache = {}

    def __init__(self, tile_size, device):
        self.tile_size = int(tile_size)
        self.device = torch.device(device)
        n = atlas_bytes(self.tile_size)
        self.tiles = torch.empty(n, dtype=torch.uint8, device=self.device).view(MG_RENDER_TILES, self.tile_size,
                                                                                 self.tile_size, 3)
        call("mg_render_build_atlas", self.device, self.tile_size, ptr(self.tiles, torch.uint8))
        # frames may be rendered on any stream later: the atlas is complete before the constructor returns
        torch.cuda.current_stream(self.device).synchronize()

    @classmethod
    def get(cls, tile_size, device):
        device = torch.device(device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        key = (device.index, int(tile_size))
        if key not in cls._cache:
            cls._cache[key] = cls(tile_size, device)
        return cls._cache[key]


def render(type_plane, colour_plane, state_plane, width, height, agent_x, agent_y, agent_dir, tile_size, highlight=None,
           env_index=None, out=None, error=None):
    """-> uint8[n, H*ts, W*ts, 3], the frames of Grid.render.  Planes uint8[N, H*W] (state_plane, highlight may be
    None); agent_* int32 device tensors, dense or the column views of the engine's records (_marshal.agent_arrays);
    env_index int32[n] picks the envs to draw (None = all); error int32[n] receives 1 where a world holds a cell that is
    not drawn (lava, unknown codes)."""
    N = type_plane.shape[0]
    W, H, ts = int(width), int(height), int(tile_size)
    assert type_plane.shape == (N, W * H) and colour_plane.shape == (N, W * H)
    dev = type_plane.device
    n = N if env_index is None else env_index.shape[0]
    frame = out if out is not None else torch.empty((n, H * ts, W * ts, 3), dtype=torch.uint8, device=dev)
    assert frame.shape == (n, H * ts, W * ts, 3) and agent_x.shape[0] >= N
    atlas = TileAtlas.get(ts, dev)
    call("mg_render", dev, ptr(type_plane, torch.uint8), ptr(colour_plane, torch.uint8), ptr(state_plane, torch.uint8), N,
         W, H, *agent_arrays(agent_x, agent_y, agent_dir), ptr(env_index, torch.int32), n, ptr(highlight, torch.uint8),
         ptr(atlas.tiles, torch.uint8), ts, ptr(frame, torch.uint8), 0, ptr(error, torch.int32))
    return frame


def render_pov(type_plane, colour_plane, state_plane, width, height, agent_x, agent_y, agent_dir, view_size, tile_size,
               carrying=None, vis_mask=None, env_index=None, out=None, error=None, see_through_walls=True):
    """-> uint8[n, V*ts, V*ts, 3], the frames of get_pov_render: the agent's V x V view drawn unmasked, the carried
    object (carrying uint8[N, 3], None = nothing) under the agent, the cells of vis_mask (uint8[N, V, V] from gen_obs)
    highlighted.  vis_mask None: every cell, or with see_through_walls=False the mask of one mg_gen_obs launch (dense
    agent arrays only).  The other arguments as in render; error also counts the carried object."""
    N = type_plane.shape[0]
    W, H, V, ts = int(width), int(height), int(view_size), int(tile_size)
    assert type_plane.shape == (N, W * H) and colour_plane.shape == (N, W * H)
    dev = type_plane.device
    n = N if env_index is None else env_index.shape[0]
    frame = out if out is not None else torch.empty((n, V * ts, V * ts, 3), dtype=torch.uint8, device=dev)
    assert frame.shape == (n, V * ts, V * ts, 3) and agent_x.shape[0] >= N
    assert carrying is None or carrying.shape == (N, 3)
    atlas = TileAtlas.get(ts, dev)
    if vis_mask is None and not see_through_walls:
        from . import minigrid_view
        vis_mask = minigrid_view.gen_obs(type_plane, colour_plane, state_plane, W, H, agent_x, agent_y, agent_dir, V,
                                         see_through_walls=False, carrying=carrying)[1]
    assert vis_mask is None or vis_mask.shape == (N, V, V)
    call("mg_render_pov", dev, ptr(type_plane, torch.uint8), ptr(colour_plane, torch.uint8), ptr(state_plane, torch.uint8),
         N, W, H, *agent_arrays(agent_x, agent_y, agent_dir), ptr(carrying, torch.uint8), ptr(env_index, torch.int32), n,
         ptr(vis_mask, torch.uint8), V, ptr(atlas.tiles, torch.uint8), ts, ptr(frame, torch.uint8), 0,
         ptr(error, torch.int32))
    return frame


def highlight_mask(vis_mask, width, height, agent_x, agent_y, agent_dir, view_size, n_envs=None, out=None):
    """get_full_render's highlight loop: vis_mask uint8[N, V, V] from gen_obs (None = every view cell visible) ->
    uint8[N, H*W] in world coordinates."""
    N = vis_mask.shape[0] if vis_mask is not None else int(n_envs)
    dev = agent_x.device
    mask = out if out is not None else torch.empty((N, int(width) * int(height)), dtype=torch.uint8, device=dev)
    assert mask.shape == (N, int(width) * int(height)) and agent_x.shape[0] >= N
    call("mg_highlight_mask", dev, ptr(vis_mask, torch.uint8), N, int(width), int(height),
         *agent_arrays(agent_x, agent_y, agent_dir), int(view_size), ptr(mask, torch.uint8))
    return mask

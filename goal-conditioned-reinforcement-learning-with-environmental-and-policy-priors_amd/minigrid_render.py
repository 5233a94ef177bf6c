"""Torch front end of the device renderer (include/minigrid_render.h): MiniGridEnv.get_full_render and get_pov_render
of the reference (gym_minigrid/minigrid.py:662-747, 1498-1563 and rendering.py) for N worlds kept as
structure-of-arrays planes on the GPU, byte for byte.  A tile atlas is rasterised once per (device, tile size); a frame
is then a gather from it.  No CPU fallback."""
import ctypes as C

import torch

from . import _lib

MG_RENDER_TILES = 600
MG_RENDER_MAX_TILE = 256


def _p(t, dtype):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous() and t.dtype == dtype, "expected contiguous %s device tensor" % dtype
    return C.c_void_p(t.data_ptr())


def _ap(t, stride):
    """Agent arrays: int32 device tensors; with a stride other than 1 only the base address is taken (e.g. a column
    view of the engine's records)."""
    assert t.is_cuda and t.dtype == torch.int32 and (stride != 1 or t.is_contiguous())
    return C.c_void_p(t.data_ptr())


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


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
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mg_render_build_atlas(self.tile_size, _p(self.tiles, torch.uint8), _stream(self.device)),
                       "mg_render_build_atlas")
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
           env_index=None, out=None, error=None, agent_stride=1):
    """-> uint8[n, H*ts, W*ts, 3], the frames of Grid.render.  Planes uint8[N, H*W] (state_plane, highlight may be
    None); agent_* int32 device tensors read at [e * agent_stride]; env_index int32[n] picks the envs to draw (None =
    all); error int32[n] receives 1 where a world holds a cell that is not drawn (lava, unknown codes)."""
    N = type_plane.shape[0]
    W, H, ts = int(width), int(height), int(tile_size)
    assert type_plane.shape == (N, W * H) and colour_plane.shape == (N, W * H)
    dev = type_plane.device
    n = N if env_index is None else env_index.shape[0]
    frame = out if out is not None else torch.empty((n, H * ts, W * ts, 3), dtype=torch.uint8, device=dev)
    assert frame.shape == (n, H * ts, W * ts, 3)
    if agent_stride == 1:
        assert agent_x.numel() >= N and agent_y.numel() >= N and agent_dir.numel() >= N
    atlas = TileAtlas.get(ts, dev)
    with torch.cuda.device(dev):                    # the launch goes to the planes' device, whichever is current
        _lib.check(_lib.lib().mg_render(
            _p(type_plane, torch.uint8), _p(colour_plane, torch.uint8), _p(state_plane, torch.uint8), N, W, H,
            _ap(agent_x, agent_stride), _ap(agent_y, agent_stride), _ap(agent_dir, agent_stride), int(agent_stride),
            _p(env_index, torch.int32), n, _p(highlight, torch.uint8), _p(atlas.tiles, torch.uint8), ts,
            _p(frame, torch.uint8), 0, _p(error, torch.int32), _stream(dev)), "mg_render")
    return frame


def render_pov(type_plane, colour_plane, state_plane, width, height, agent_x, agent_y, agent_dir, view_size, tile_size,
               carrying=None, vis_mask=None, env_index=None, out=None, error=None, agent_stride=1, see_through_walls=True):
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
    assert frame.shape == (n, V * ts, V * ts, 3)
    assert carrying is None or carrying.shape == (N, 3)
    if agent_stride == 1:
        assert agent_x.numel() >= N and agent_y.numel() >= N and agent_dir.numel() >= N
    atlas = TileAtlas.get(ts, dev)
    with torch.cuda.device(dev):
        if vis_mask is None and not see_through_walls:
            from . import minigrid_view
            assert agent_stride == 1, "mg_gen_obs reads dense agent arrays"
            vis_mask = minigrid_view.gen_obs(type_plane, colour_plane, state_plane, W, H, agent_x, agent_y, agent_dir, V,
                                             see_through_walls=False, carrying=carrying)[1]
        assert vis_mask is None or vis_mask.shape == (N, V, V)
        _lib.check(_lib.lib().mg_render_pov(
            _p(type_plane, torch.uint8), _p(colour_plane, torch.uint8), _p(state_plane, torch.uint8), N, W, H,
            _ap(agent_x, agent_stride), _ap(agent_y, agent_stride), _ap(agent_dir, agent_stride), int(agent_stride),
            _p(carrying, torch.uint8), _p(env_index, torch.int32), n, _p(vis_mask, torch.uint8), V,
            _p(atlas.tiles, torch.uint8), ts, _p(frame, torch.uint8), 0, _p(error, torch.int32), _stream(dev)),
            "mg_render_pov")
    return frame


def highlight_mask(vis_mask, width, height, agent_x, agent_y, agent_dir, view_size, n_envs=None, agent_stride=1, out=None):
    """get_full_render's highlight loop: vis_mask uint8[N, V, V] from gen_obs (None = every view cell visible) ->
    uint8[N, H*W] in world coordinates."""
    N = vis_mask.shape[0] if vis_mask is not None else int(n_envs)
    dev = agent_x.device
    mask = out if out is not None else torch.empty((N, int(width) * int(height)), dtype=torch.uint8, device=dev)
    assert mask.shape == (N, int(width) * int(height))
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().mg_highlight_mask(
            _p(vis_mask, torch.uint8), N, int(width), int(height), _ap(agent_x, agent_stride), _ap(agent_y, agent_stride),
            _ap(agent_dir, agent_stride), int(agent_stride), int(view_size), _p(mask, torch.uint8), _stream(dev)),
            "mg_highlight_mask")
    return mask

"""TwoarmyEngine: torch-tensor front end of the HIP engine handle (include/twoarmy.h).

PyTorch is plumbing here (device memory + streams); all env compute is in libtwoarmy_hip.so.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._marshal import constant, inner, ptr, stream
from ._lib import (FIELDS, TW_CELLS, TW_DRAW_WORDS, TW_F_AUTORESET, TW_F_MATRIX_CODE, TW_F_POLICY_IDX, TW_F_SLAB_HIPMALLOC,
                   TW_REC_WORDS)

REWARD_VALUES = (-0.01, -0.1, -0.9, 0.2, 0.9)
MAT_PITCH = 292                       # floats per env matrix in the native layout (289 + 3 zero pad)
MATC_PITCH = 304                      # bytes per env matrix in the code layout (TW_F_MATRIX_CODE; 289 + 15 pad)
MATRIX_CODE_VALUES = (0.9, -0.9, -0.5, 0.3)     # code -> Env_transact.matrix_env value (free/goal, wall, ball, agent)


def obs_pitch_for(view):
    """Bytes per env image in the native layout: V*V*3 rounded up to 16 (880 for V=17)."""
    return (view * view * 3 + 15) // 16 * 16


def _pitched(t, lead, inner_shape, dtype):
    """(pointer, pitch in elements) of a [*lead, *inner_shape] tensor whose rows may be padded."""
    if t is None:
        return None, 0
    assert t.is_cuda and t.dtype == dtype, "expected %s device tensor" % dtype
    nlead = len(lead)
    assert tuple(t.shape) == tuple(lead) + tuple(inner_shape), (tuple(t.shape), lead, inner_shape)
    row = inner(t, nlead)
    # row pitch from the innermost leading dim of size > 1 (strides of size-1 dims are arbitrary)
    pitch, mult = None, 1
    for d in range(nlead - 1, -1, -1):
        if t.shape[d] > 1:
            if pitch is None:
                assert t.stride(d) % mult == 0
                pitch = t.stride(d) // mult
            else:
                assert t.stride(d) == pitch * mult, "leading dims must be dense"
        mult *= t.shape[d]
    if pitch is None:
        pitch = row
    assert pitch >= row
    return C.c_void_p(t.data_ptr()), int(pitch)


def padded_rows(t, nlead, width):
    """The padded rows behind a native-layout output: [*lead, width] view of every row including its pad bytes /
    floats (t is the [*lead, ...] strided view handed out by alloc_outputs; nlead = len(lead); width = 880 / 292 / 304)."""
    lead = tuple(t.shape[:nlead])
    assert width <= t.stride(nlead - 1)
    strides = tuple(t.stride(d) for d in range(nlead)) + (1,)
    return t.as_strided(lead + (width,), strides)


class _DevSpan:
    """A span of a library-owned device slab, exported through __cuda_array_interface__ so that torch wraps it without
    copying; torch keeps this object (and through it the slab) alive as long as any view of the tensor lives."""

    def __init__(self, owner, ptr, nbytes):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (int(ptr), False),
                                         "version": 2, "strides": None}


class _OutputSlab:
    """One tw_alloc_outputs slab; freed (tw_free_outputs) when the last tensor carved from it is gone."""

    def __init__(self, engine, T, flags):
        self.out = _lib.TwOutputs()
        self.device = engine.device
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().tw_alloc_outputs(engine._h, int(T), int(flags), C.byref(self.out)), "tw_alloc_outputs")
        self.backing = int(self.out.backing)

    def tensor(self, addr, nbytes, dtype):
        t = torch.as_tensor(_DevSpan(self, addr, nbytes), device=self.device)
        if t.data_ptr() != int(addr) or t.device != self.device:
            raise _lib.TwoarmyLibraryError("torch did not alias the engine slab (got %s at %#x for %#x on %s)"
                                           % (t.device, t.data_ptr(), int(addr), self.device))
        return t.view(dtype)

    def __del__(self):
        try:
            if self.out.slab:
                rc = _lib.lib().tw_free_outputs(C.byref(self.out))
                if rc != 0:
                    import sys
                    print("tw_free_outputs failed: rc=%d %s" % (rc, _lib.lib().tw_last_error_message().decode()), file=sys.stderr)
        except Exception:
            pass


class TwoarmyEngine:
    """N independent MiniGrid-Twoarmy envs living in HBM on one GPU.

    variant: "v4"/4 (hard) or "v6"/6 (easy) -- gym ids MiniGrid-twoarmy-17x17-v{4,6}
    (reference gym_minigrid/__init__.py:6-21).
    """

    def __init__(self, variant, num_envs, view_size=17, device=None, seed=9981, env_id0=0, max_steps=50):
        variant = {"v4": 4, "v6": 6}.get(variant, variant)
        if not torch.cuda.is_available():
            raise _lib.TwoarmyLibraryError("TwoarmyEngine needs a GPU (no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.variant, self.num_envs, self.view_size = variant, int(num_envs), int(view_size)
        self.seed, self.env_id0 = int(seed), int(env_id0)
        self._h, self._own_views = C.c_void_p(), None
        lib = _lib.lib()
        with torch.cuda.device(self.device):
            torch.cuda.current_stream().synchronize()
            _lib.check(lib.tw_create(C.byref(self._h), variant, self.num_envs, self.view_size,
                                     self.device.index or 0, self.seed, self.env_id0), "tw_create")
        self.max_steps = int(max_steps)
        if self.max_steps != 50:              # MiniGridEnv(max_steps=...) (minigrid.py:866-945; Twoarmy passes 50)
            if self.max_steps <= 0:
                raise ValueError("max_steps must be positive")
            _, _, rec = self.get_state()
            rec[:, FIELDS["MAX_STEPS"]] = self.max_steps
            self.set_state(records=rec)

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            _lib.lib().tw_destroy(self._h)
            self._h = self._own_views = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_pipeline(self, enable):
        """False: the sequential kernel only; True: the pipelined kernel where eligible; 2: the same, with the state
        pinned (pin_state)."""
        _lib.check(_lib.lib().tw_set_pipeline(self._h, 2 if enable == 2 else int(bool(enable))), "tw_set_pipeline")

    def pin_state(self):
        """Keep the state where it is for good (tw_set_pipeline(e, 2), include/twoarmy.h): pipelined rollouts then copy
        the ping-pong partner back on the stream instead of swapping the buffers, so graphs that hold a launch of this
        engine, and the views of plane_views() / agent_views(), stay valid across them.  A captured pipelined rollout
        pins the engine by itself; pin before capturing step(), reset() or gen_obs() of an engine that also runs eager
        pipelined rollouts."""
        self.set_pipeline(2)

    def fallback_count(self):
        """Pipelined launches re-run by the sequential fallback so far (0 in normal play)."""
        n = C.c_int()
        _lib.check(_lib.lib().tw_fallback_count(self._h, C.byref(n)), "tw_fallback_count")
        return n.value

    def last_launch(self):
        """What the most recent step / rollout launched (tw_last_launch): {pipelined, PG, LAYOUT, pipe_grid, E, FAST,
        seq_grid, T}; with pipelined = 1 the sequential fields describe the fallback launch behind the pipelined kernel."""
        info = (C.c_int * len(_lib.LAUNCH_FIELDS))()
        _lib.check(_lib.lib().tw_last_launch(self._h, info), "tw_last_launch")
        return dict(zip(_lib.LAUNCH_FIELDS, info))

    def set_envs_per_wave(self, e):
        _lib.check(_lib.lib().tw_set_envs_per_wave(self._h, int(e)), "tw_set_envs_per_wave")

    # ------------------------------------------------------------------ buffers
    def alloc_outputs(self, T=None, obs=True, matrix=True, dense=False, matrix_codes=False, slab=None):
        """Output tensors for step (T=None -> [N,...]) or rollout ([T,N,...]).

        Native layout (dense=False): obs rows padded to 16 bytes (880 for V=17) and matrix rows to
        292 floats; the returned tensors are [..., V, V, 3] / [..., 289] strided views of them.
        matrix_codes=True: the matrix is uint8 codes (rows of 304 bytes natively), see TW_F_MATRIX_CODE;
        a uint8 matrix tensor selects that mode in step/rollout.
        slab (default: on for the native layout with every output): the buffers are carved out of ONE slab the
        library allocates (tw_alloc_outputs) -- the same placement for every user of the C ABI; the tensors keep the
        slab alive.  slab=False takes them from torch's caching allocator; slab="hipmalloc" asks for a slab backed by
        plain hipMalloc memory (TW_F_SLAB_HIPMALLOC) instead of mapped 2 MiB chunks."""
        N, V = self.num_envs, self.view_size
        lead = (N,) if T is None else (T, N)
        d = self.device
        nb = V * V * 3
        if slab is None:
            slab = (not dense) and obs and matrix
        if slab:
            assert not dense and obs and matrix, "the engine slab holds the native layout with every output"
            assert slab is True or slab == "hipmalloc", slab
            return self._slab_outputs(T, lead, matrix_codes, hipmalloc=slab == "hipmalloc")
        if dense:
            o = torch.empty(lead + (V, V, 3), dtype=torch.uint8, device=d) if obs else None
            m = torch.empty(lead + (TW_CELLS,), dtype=torch.uint8 if matrix_codes else torch.float32, device=d) \
                if matrix else None
        else:
            o = torch.empty(lead + (obs_pitch_for(V),), dtype=torch.uint8, device=d)[..., :nb].view(lead + (V, V, 3)) \
                if obs else None
            if not matrix:
                m = None
            elif matrix_codes:
                m = torch.empty(lead + (MATC_PITCH,), dtype=torch.uint8, device=d)[..., :TW_CELLS]
            else:
                m = torch.empty(lead + (MAT_PITCH,), dtype=torch.float32, device=d)[..., :TW_CELLS]
        return dict(
            obs=o, matrix=m,
            pos=torch.empty(lead + (2,), dtype=torch.float32, device=d),
            reward=torch.empty(lead, dtype=torch.float32, device=d),
            terminated=torch.empty(lead, dtype=torch.uint8, device=d),
            truncated=torch.empty(lead, dtype=torch.uint8, device=d),
        )

    def _slab_outputs(self, T, lead, matrix_codes, hipmalloc=False):
        N, V = self.num_envs, self.view_size
        flags = (TW_F_MATRIX_CODE if matrix_codes else 0) | (TW_F_SLAB_HIPMALLOC if hipmalloc else 0)
        owner = _OutputSlab(self, 1 if T is None else T, flags)
        fell_back = False
        try:
            owner.tensor(min(owner.out.obs, owner.out.matrix), 16, torch.uint8)
        except _lib.TwoarmyLibraryError as exc:
            # a mapped slab torch cannot wrap in place (seen nowhere so far; multi-GPU ranks are the untested case):
            # the same layout from plain hipMalloc memory, whose pointer attributes torch certainly understands.
            # Never silent: a warning here, `_tw_fallback` on the tensors, `config.slab_backing` in bench.py's line
            # (ranks that disagree abort the run), TW_SLAB_STRICT=1 turns it into an error.
            import os
            import warnings
            if os.environ.get("TW_SLAB_STRICT", "0") == "1":
                raise
            warnings.warn("engine slab: falling back to hipMalloc backing (%s)" % exc, RuntimeWarning)
            fell_back = True
            owner = _OutputSlab(self, 1 if T is None else T, flags | TW_F_SLAB_HIPMALLOC)
        o = owner.out
        TN = (1 if T is None else T) * N
        nb = V * V * 3
        # one stream of records (include/twoarmy.h): float frames = matrix row | image row, code frames = image row | code row
        rb = int(o.obs_pitch)
        rec = owner.tensor(min(o.obs, o.matrix), TN * rb, torch.uint8).view(lead + (rb,))
        orow = obs_pitch_for(V)
        if matrix_codes:
            assert o.matrix == o.obs + orow and o.mat_pitch == rb == orow + MATC_PITCH
            obs = rec[..., :nb].view(lead + (V, V, 3))
            m = rec[..., orow:orow + TW_CELLS]
        else:
            assert o.obs == o.matrix + MAT_PITCH * 4 and o.mat_pitch * 4 == rb == MAT_PITCH * 4 + orow
            m = rec[..., :MAT_PITCH * 4].view(torch.float32)[..., :TW_CELLS]
            obs = rec[..., MAT_PITCH * 4:MAT_PITCH * 4 + nb].view(lead + (V, V, 3))
        m._tw_layout = ("%d-byte records (image | codes)" % rb if matrix_codes else "%d-byte records (matrix | image)" % rb) + \
            (", hipMalloc" if o.backing == 0 else ", 2 MiB mapped chunks")
        m._tw_fallback = fell_back
        return dict(obs=obs, matrix=m,
                    pos=owner.tensor(o.pos, TN * 8, torch.float32).view(lead + (2,)),
                    reward=owner.tensor(o.reward, TN * 4, torch.float32).view(lead),
                    terminated=owner.tensor(o.terminated, TN, torch.uint8).view(lead),
                    truncated=owner.tensor(o.truncated, TN, torch.uint8).view(lead))

    # ------------------------------------------------------------------ ops
    def reset(self, mask=None, obs=None):
        V = self.view_size
        op, opitch = _pitched(obs, (self.num_envs,), (V, V, 3), torch.uint8)
        _lib.check(_lib.lib().tw_reset(self._h, ptr(mask, torch.uint8), op, opitch, stream(self.device)), "tw_reset")
        return obs

    @staticmethod
    def _matrix_arg(m, lead, flags):
        """(pointer, pitch, flags): a uint8 matrix tensor means code frames (pitch in bytes)."""
        if m is not None and m.dtype == torch.uint8:
            mp, mpitch = _pitched(m, lead, (TW_CELLS,), torch.uint8)
            return mp, mpitch, flags | TW_F_MATRIX_CODE
        mp, mpitch = _pitched(m, lead, (TW_CELLS,), torch.float32)
        return mp, mpitch, flags

    @staticmethod
    def decode_matrix(codes):
        """uint8 code frames -> the float matrix of Env_transact.matrix_env (env_buffer.py:300-336)."""
        lut = constant("matrix_code_values", MATRIX_CODE_VALUES, torch.float32, codes.device)
        return lut[codes.long()]

    def _out_args(self, lead, out, flags):
        """(obs, obs_pitch, matrix, mat_pitch, pos, reward, terminated, truncated), flags: the output arguments of a launch."""
        V = self.view_size
        op, opitch = _pitched(out.get("obs"), lead, (V, V, 3), torch.uint8)
        mp, mpitch, flags = self._matrix_arg(out.get("matrix"), lead, flags)
        for k, dt in (("pos", torch.float32), ("reward", torch.float32), ("terminated", torch.uint8),
                      ("truncated", torch.uint8)):
            t = out.get(k)
            assert t is None or (t.is_contiguous() and t.dtype == dt and tuple(t.shape[:len(lead)]) == lead), k
        return [op, opitch, mp, mpitch, ptr(out.get("pos")), ptr(out.get("reward")), ptr(out.get("terminated")),
                ptr(out.get("truncated"))], flags

    def _launch(self, fn, name, lead, T, actions, draws, out, flags):
        outs, flags = self._out_args(lead, out, flags)
        args = [self._h] + ([T] if T is not None else []) + [ptr(actions, torch.int32), ptr(draws)] + outs + [
            flags, stream(self.device)]
        _lib.check(fn(*args), name)
        return out

    def step(self, actions, out, draws=None, autoreset=False, policy_idx=False):
        flags = (TW_F_AUTORESET if autoreset else 0) | (TW_F_POLICY_IDX if policy_idx else 0)
        assert actions.shape == (self.num_envs,)
        if draws is not None:
            assert draws.shape == (self.num_envs, TW_DRAW_WORDS) and draws.dtype == torch.int32 and draws.is_contiguous()
        return self._launch(_lib.lib().tw_step, "tw_step", (self.num_envs,), None, actions, draws, out, flags)

    def rollout(self, T, out, actions=None, draws=None, autoreset=True, policy_idx=True):
        """T steps in one launch on the current stream.  May be captured in a graph: a pipelined launch (T >= 8 with
        auto-reset) on a capturing stream pins the state (pin_state) and copies it back on the stream from then on."""
        flags = (TW_F_AUTORESET if autoreset else 0) | (TW_F_POLICY_IDX if policy_idx else 0)
        if actions is not None:
            assert actions.shape == (T, self.num_envs)
        if draws is not None:
            assert draws.shape == (T, self.num_envs, TW_DRAW_WORDS) and draws.dtype == torch.int32 and draws.is_contiguous()
        return self._launch(_lib.lib().tw_rollout, "tw_rollout", (T, self.num_envs), T, actions, draws, out, flags)

    def fill_actions(self, T):
        a = torch.empty((T, self.num_envs), dtype=torch.int32, device=self.device)
        _lib.check(_lib.lib().tw_fill_actions(self._h, T, ptr(a), stream(self.device)), "tw_fill_actions")
        return a

    def gen_obs(self, view_size=None):
        V = view_size or self.view_size
        obs = torch.empty((self.num_envs, V, V, 3), dtype=torch.uint8, device=self.device)
        _lib.check(_lib.lib().tw_gen_obs(self._h, V, ptr(obs), 0, stream(self.device)), "tw_gen_obs")
        return obs

    def render(self, env_index=None, tile_size=17, highlight=False, out=None):
        """RGB frames of MiniGridEnv.get_full_render, uint8[n, 17*ts, 17*ts, 3], drawn on the device straight from the
        engine's planes and records (tw_state_ptrs) on the current stream: no host copy of the state.  env_index:
        int32 device tensor of the envs to draw (None = all); highlight: brighten the agent's view_size x view_size
        view as the reference's `highlight=True` does (Twoarmy sees through walls: the whole view)."""
        from . import minigrid_render as mr
        ty, co, agent = self._views()
        hm = mr.highlight_mask(None, 17, 17, *agent, self.view_size, n_envs=self.num_envs) if highlight else None
        return mr.render(ty, co, None, 17, 17, *agent, tile_size, highlight=hm, env_index=env_index, out=out)

    def render_pov(self, env_index=None, tile_size=17, view_size=None, out=None):
        """RGB frames of MiniGridEnv.get_pov_render, uint8[n, V*ts, V*ts, 3] (V = view_size, default the engine's):
        the agent's view with the agent at the bottom centre pointing up, every cell highlighted (Twoarmy sees through
        walls and carries nothing).  Drawn like render(): from the engine's planes and records, on the current stream."""
        from . import minigrid_render as mr
        ty, co, agent = self._views()
        return mr.render_pov(ty, co, None, 17, 17, *agent, view_size or self.view_size, tile_size, env_index=env_index,
                             out=out)

    def _state_ptrs(self):
        """(type planes, colour planes, records): device addresses of the engine's state as it stands.  A pipelined
        rollout (T >= 8 with auto-reset) writes the ping-pong partner and swaps the two, so ask again after one."""
        ty, co, rec = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _lib.check(_lib.lib().tw_state_ptrs(self._h, C.byref(ty), C.byref(co), C.byref(rec)), "tw_state_ptrs")
        return ty.value, co.value, rec.value

    def _views(self, owner=None):
        """(type, colour) uint8[N, 289] and the (TW_AX, TW_AY, TW_DIR) columns of the records as int32 [N,
        TW_REC_WORDS]: device views of the engine's own state (no copy).  Views that are handed out keep `owner` (the
        engine) alive; render(), render_pov() and distance_field() use one set of their own, rebuilt when a pipelined
        rollout has swapped the state's buffers."""
        addrs = self._state_ptrs()                     # a pipelined rollout swaps the state with its ping-pong partner
        if owner is None and self._own_views is not None and self._own_views[0] == addrs:
            return self._own_views[1]
        N, flat = self.num_envs, []
        for addr, nbytes in zip(addrs, (N * TW_CELLS, N * TW_CELLS, N * TW_REC_WORDS * 4)):
            t = torch.as_tensor(_DevSpan(owner, addr, nbytes), device=self.device)
            if t.data_ptr() != addr:
                raise _lib.TwoarmyLibraryError("torch did not alias the engine's state")
            flat.append(t)
        rec = flat[2].view(torch.int32).view(N, TW_REC_WORDS)
        views = (flat[0].view(N, TW_CELLS), flat[1].view(N, TW_CELLS), tuple(rec[:, FIELDS[k]] for k in ("AX", "AY", "DIR")))
        if owner is None:
            self._own_views = (addrs, views)
        return views

    def dir_ptr(self):
        """(address, stride_t, stride_n) of the agents' directions in the engine's records (tw_state_ptrs), in int32
        elements: one value per env, as ppo_ops.bonus_scan(dir_ptr=...) takes it.  After an auto-reset the record holds
        the new episode's direction."""
        return self._state_ptrs()[2] + 4 * FIELDS["DIR"], 0, TW_REC_WORDS

    def plane_views(self):
        """(type, colour) uint8[N, 289] device views of the engine's own planes (tw_state_ptrs; no copy): cell (x, y)
        at y*17 + x.  They show the state of the moment a kernel reads them, until a pipelined rollout (T >= 8 with
        auto-reset) swaps the buffers: take new views after one.  step() and shorter rollouts write in place."""
        return self._views(self)[:2]

    def agent_views(self):
        """(x, y, dir) int32[N] strided device views of TW_AX, TW_AY and TW_DIR in the engine's records (no copy): the
        agent_* arguments of minigrid_obs and minigrid_render, which then read the agent where it lives."""
        return self._views(self)[2]

    def dir_view(self):
        """int32[N] strided device view of the same directions (no copy)."""
        return self.agent_views()[2]

    def distance_field(self, goal=None, pass_types=None, agent=True, out=None, want_field=True, agent_out=None,
                       error_out=None):
        """Shortest-path distances of the engine's worlds as they stand (minigrid_nav.distance_field, one launch, read
        from the engine's own planes and records: no gather pass, no host copy) -> (dist uint16[N, 289] or None,
        agent_dist int32[N], agent_action int32[N], error int32[N]).  goal: (x, y) int32[N] device tensors, None = the
        goal cell of the plane; pass_types: minigrid_nav.PASS_DEFAULT (what the agent may step on now: balls and
        patrols block) or | PASS_BALL for the static map; want_field=False: the agent's two values only; agent_out =
        (agent_dist, agent_action), error_out: int32[N] tensors to write into.  Twoarmy has no doors, hence no state
        plane."""
        from . import minigrid_nav as nav
        ty, _, ag = self._views()
        return nav.distance_field(ty, None, 17, 17, nav.PASS_DEFAULT if pass_types is None else pass_types, goal=goal,
                                  agent=ag[:2] if agent else None, out=out, want_field=want_field,
                                  agent_out=agent_out, error_out=error_out)

    def timed_field(self, avoid_risk=False, goal=None, agent=True, out=None, want_field=True, agent_out=None,
                    error_out=None):
        """Time-expanded shortest paths of the engine's worlds (minigrid_nav.timed_field, one launch, read from the
        engine's own planes and the AX / AY / STEP_MOVE words of its records) -> (dist uint16[N, 6, 289] or None,
        agent_dist int32[N], agent_action int32[N], error int32[N]).  The row-8 balls are planned by their period-6
        schedule (minigrid_nav.twoarmy_schedule; phase = step_move % 6), so the expert waits for the gap to open
        instead of walking into a ball: agent_action 6 off the goal means "wait one step".  avoid_risk: also keep out
        of the -0.1 cell under each ball.  The plane's own balls are passable (PASS_BALL): only the schedule blocks.
        v6: the two constant 2x2 wall blocks are planned as present from the reset on (they appear with the agent's
        first step out of the start corner, and no block cell touches a corner cell), so one field at a reset serves the
        whole episode, exactly.  v4: the blocks are drawn at random and the patrol groups move behind RNG gates: the
        field plans on the planes as they stand (blocks once they have dropped) and does NOT schedule the patrols --
        their balls are passable, as in the static prior.  The other arguments as in distance_field."""
        from . import minigrid_nav as nav
        ty, _, ag = self._views()
        blocked = self._schedule(avoid_risk, ty.device)
        clock = ag[0].as_strided(ag[0].shape, ag[0].stride(), ag[0].storage_offset() + FIELDS["STEP_MOVE"] - FIELDS["AX"])
        return nav.timed_field(ty, None, 17, 17, blocked, nav.PASS_DEFAULT | nav.PASS_BALL, goal=goal,
                               agent=ag[:2] if agent else None, clock=clock if agent else None, out=out,
                               want_field=want_field, agent_out=agent_out, error_out=error_out)

    def _schedule(self, avoid_risk, device):
        """The cached minigrid_nav.twoarmy_schedule of this variant on `device`."""
        from . import minigrid_nav as nav
        key = (bool(avoid_risk), device)
        if getattr(self, "_schedules", None) is None:
            self._schedules = {}
        if key not in self._schedules:
            self._schedules[key] = nav.twoarmy_schedule(avoid_risk, blocks=self.variant == 6, device=device)
        return self._schedules[key]

    def _her_args(self, her, pass_types=None, timed=False, avoid_risk=False):
        """What the *_goal_* methods hand minigrid_nav -> (nav, (type plane, t, n, goal), keywords): the engine's own plane
        and the records' columns; pass_types (None: PASS_DEFAULT), or for the timed ones PASS_BALL on top and the cached
        schedule as `blocked`."""
        from . import minigrid_nav as nav
        ty = self._views()[0]
        kw = {"pass_types": nav.PASS_DEFAULT if pass_types is None else pass_types}
        if timed:
            kw = {"pass_types": nav.PASS_DEFAULT | nav.PASS_BALL, "blocked": self._schedule(avoid_risk, ty.device)}
        return nav, (ty, her["t"], her["n"], her["goal"]), kw

    def goal_moves(self, her, pos, age=None, init_pos=None, pass_types=None, out=None, dist_out=None):
        """Optimal-move sets of hindsight records under their own goals in the engine's worlds as they stand
        (minigrid_nav.goal_moves, one launch, read from the engine's own planes) -> (moves uint8[R], acting_dist
        uint16[R]).  her: the records of ppo_ops.her_relabel (its "t", "n" and "goal"); pos float32[T, N, 2] BEFORE each
        step, age int32[T, N] and init_pos float32[2] as minigrid_nav.optimal_moves takes them; pass_types as in
        distance_field."""
        nav, rec, kw = self._her_args(her, pass_types)
        return nav.goal_moves(*rec, pos, 17, 17, age=age, init_pos=init_pos, out=out, dist_out=dist_out, **kw)

    def goal_ahead(self, her, pos, age=None, init_pos=None, steps=3, pass_types=None, out=None, dist_out=None):
        """Look-ahead labels of hindsight records under their own goals in the engine's worlds as they stand
        (minigrid_nav.goal_ahead, one launch, read from the engine's own planes) -> (labels int64[R], acting_dist
        uint16[R]): where a shortest path to the record's goal stands `steps` steps after the record's acting state.
        her, pos, age, init_pos and pass_types as goal_moves takes them."""
        nav, rec, kw = self._her_args(her, pass_types)
        return nav.goal_ahead(*rec, pos, 17, 17, steps=steps, age=age, init_pos=init_pos, out=out, dist_out=dist_out, **kw)

    def goal_shape(self, her, pos_before, pos_after, age=None, init_pos=None, pass_types=None, scale=1.0, gamma=0.99,
                   zero_terminal=False, out=None, shaping_out=None, mask_out=None):
        """Potential-based shaping of hindsight records under their own goals in the engine's worlds as they stand
        (minigrid_nav.goal_shape, one launch, read from the engine's own planes) -> (reward' float32[R], F float32[R],
        mask uint8[R]).  her: the records of ppo_ops.her_relabel (its "t", "n", "goal", "reward" and "done"); pos_before /
        pos_after float32[T, N, 2], age int32[T, N] and init_pos float32[2] as minigrid_nav.shape takes them; pass_types
        as in distance_field; out=her["reward"] shapes the records in place."""
        nav, rec, kw = self._her_args(her, pass_types)
        return nav.goal_shape(*rec, pos_before, pos_after, 17, 17, reward=her["reward"], done=her["done"], age=age,
                              init_pos=init_pos, scale=scale, gamma=gamma, zero_terminal=zero_terminal, out=out,
                              shaping_out=shaping_out, mask_out=mask_out, **kw)

    def timed_goal_moves(self, her, pos, age, init_pos, avoid_risk=False, out=None, dist_out=None):
        """goal_moves over (cell, phase): the optimal-move sets of hindsight records under their own goals with the
        row-8 balls planned by their period-6 schedule (minigrid_nav.timed_goal_moves, one launch, read from the
        engine's own planes, no field in memory) -> (moves uint8[R], acting_dist uint16[R]).  her, pos, age and
        init_pos as goal_moves takes them, age and init_pos required: the age of a step is its clock, as in
        minigrid_nav.timed_moves.  The stay bit off the goal means "wait one step".  The schedule is the one
        timed_field() caches (avoid_risk as there), the plane's own balls are passable (PASS_BALL).
        v6: the two constant 2x2 wall blocks are planned as present from the reset on, as in timed_field().  That
        stays exact for hindsight goals inside the start corner as well: no block cell touches a corner cell, and a
        shortest path between two cells of the corner stays inside the corner rectangle, so the labels of a record that
        acts before the blocks have dropped, towards a goal it reached before they dropped, do not see them; every other
        record's path leaves the corner and meets the blocks in place.  v4: the caveat of timed_field() holds unchanged
        (blocks as they stand, patrols not scheduled)."""
        nav, rec, kw = self._her_args(her, timed=True, avoid_risk=avoid_risk)
        return nav.timed_goal_moves(*rec, pos, 17, 17, age=age, init_pos=init_pos, out=out, dist_out=dist_out, **kw)

    def timed_goal_ahead(self, her, pos, age, init_pos, steps=3, avoid_risk=False, out=None, dist_out=None):
        """goal_ahead over (cell, phase): the look-ahead labels of hindsight records under their own goals with the
        row-8 balls planned by their period-6 schedule (minigrid_nav.timed_goal_ahead, one launch, read from the engine's
        own planes, no field in memory) -> (labels int64[R], acting_dist uint16[R]).  her, pos, age, init_pos and steps as
        goal_ahead takes them, age and init_pos required: the age of a step is its clock.  Bit 24 off the goal means
        "wait here".  Planes and schedule exactly as timed_goal_moves takes them -- the schedule timed_field() caches
        (avoid_risk as there), the plane's own balls passable (PASS_BALL), v6's blocks planned as present from the reset
        on, v4's caveat unchanged -- so a record's label is the one minigrid_nav.ahead reads from timed_field()'s fields
        for the rollout."""
        nav, rec, kw = self._her_args(her, timed=True, avoid_risk=avoid_risk)
        return nav.timed_goal_ahead(*rec, pos, 17, 17, age=age, init_pos=init_pos, steps=steps, out=out, dist_out=dist_out,
                                    **kw)

    def timed_goal_shape(self, her, pos_before, pos_after, age, init_pos, avoid_risk=False, scale=1.0, gamma=0.99,
                         zero_terminal=False, out=None, shaping_out=None, mask_out=None):
        """goal_shape over (cell, phase): potential-based shaping of hindsight records under their own goals with the
        row-8 balls planned by their period-6 schedule (minigrid_nav.timed_goal_shape, one launch, read from the
        engine's own planes, no field in memory) -> (reward' float32[R], F float32[R], mask uint8[R]), as goal_shape
        returns them.  her, pos_before, pos_after, scale, gamma, zero_terminal and the outputs as goal_shape takes them;
        age and init_pos required: the age of a step is its clock.  Planes and schedule exactly as timed_goal_moves takes
        them -- the schedule timed_field() caches (avoid_risk as there), the plane's own balls passable (PASS_BALL), v6's
        blocks planned as present from the reset on, v4's caveat unchanged -- so a record's potential is the one
        shape() reads from timed_field()'s fields for the rollout."""
        nav, rec, kw = self._her_args(her, timed=True, avoid_risk=avoid_risk)
        return nav.timed_goal_shape(*rec, pos_before, pos_after, 17, 17, age=age, init_pos=init_pos, reward=her["reward"],
                                    done=her["done"], scale=scale, gamma=gamma, zero_terminal=zero_terminal, out=out,
                                    shaping_out=shaping_out, mask_out=mask_out, **kw)

    def time_rollout(self, T, out, actions=None, autoreset=True, iters=10):
        """Mean kernel time (ms) of one tw_rollout launch, HIP events on the current stream."""
        ms = C.c_float()
        flags = (TW_F_AUTORESET if autoreset else 0) | TW_F_POLICY_IDX
        outs, flags = self._out_args((T, self.num_envs), out, flags)
        _lib.check(_lib.lib().tw_time_rollout(self._h, T, ptr(actions, torch.int32), *outs, flags, iters,
                                              C.byref(ms), stream(self.device)), "tw_time_rollout")
        return ms.value

    # ------------------------------------------------------------------ state
    def get_state(self):
        """(type uint8[N,289], colour uint8[N,289], records int32[N,48]) as numpy (host copies)."""
        N = self.num_envs
        ty = np.empty((N, TW_CELLS), np.uint8)
        co = np.empty((N, TW_CELLS), np.uint8)
        rec = np.empty((N, TW_REC_WORDS), np.int32)
        _lib.check(_lib.lib().tw_get_state_host(self._h, ty.ctypes.data_as(C.c_void_p), co.ctypes.data_as(C.c_void_p),
                                                rec.ctypes.data_as(C.c_void_p)), "tw_get_state_host")
        return ty, co, rec

    def set_state(self, type_plane=None, colour_plane=None, records=None):
        keep = []

        def p(a, dt, shape):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt)
            assert a.shape == shape
            keep.append(a)
            return a.ctypes.data_as(C.c_void_p)
        N = self.num_envs
        _lib.check(_lib.lib().tw_set_state_host(self._h, p(type_plane, np.uint8, (N, TW_CELLS)),
                                                p(colour_plane, np.uint8, (N, TW_CELLS)),
                                                p(records, np.int32, (N, TW_REC_WORDS))), "tw_set_state_host")

    @staticmethod
    def field(records, name, k=0):
        return records[..., FIELDS[name] + k]

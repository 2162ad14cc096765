"""The kernel shapes of an env (include/dronenav.h dn_get_kernel_waves) on the HIP path, small fleets, host state only:

 1. dn_create's pick is the function tests/test_kernel_shapes_cpu.py walks: the library against the host program, on this device's num_cus;
 2. an enabled model forces the one-wave kernels, bound or not, and the fused sampling entry points refuse the env;
 3. the sampled / squashed steps and the two bind calls refuse in their documented order, with their messages word for word.

Only (2) launches anything: one dn_step per enabled-but-unbound row writer."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gpu_support import DEV  # noqa: E402
from gpu_support import pkg as _pkg  # noqa: E402
from kernel_shapes_support import build_program, run_program  # noqa: E402

INVALID = -1


@pytest.fixture(autouse=True)
def _no_overrides(monkeypatch):
    monkeypatch.delenv("DN_WAVES", raising=False)
    monkeypatch.delenv("DN_WAVES_SINGLE", raising=False)


def _capi_module():
    from drl_dronenavigation_amd import _capi
    return _capi


def _env(pkg, n, **kw):
    from drl_dronenavigation_amd import tracks
    opts = dict(normalize_obs=False, ground_contact=False, max_steps=40, device=DEV)
    opts.update(kw)
    return pkg.DroneVecEnv(tracks.circle(1, 4, 1), n, **opts)


def _shapes(env):
    return env.kernel_waves(fused=True), env.kernel_waves(fused=False)


def test_the_library_picks_what_the_host_program_prints(tmp_path):
    pkg = _pkg()
    exe = build_program(tmp_path)
    for n, kw in ((4096, dict()), (4096, dict(normalize_obs=True)), (32768, dict()), (32768, dict(normalize_obs=True)),
                  (49152, dict(clip_rew=True)), (65536, dict(ground_contact=True))):
        env = _env(pkg, n, **kw)
        keys = dict(num_cus=env.num_cus, num_envs=n, normalize_obs=int(env.cfg.normalize_obs), ground_contact=int(env.cfg.ground_contact),
                    clip_rew=int(env.cfg.clip_rew))
        assert keys["normalize_obs"] == int(bool(kw.get("normalize_obs"))) and keys["ground_contact"] == int(bool(kw.get("ground_contact")))
        want = run_program(exe, **keys)
        got = _shapes(env)
        env.close()
        assert got == (want["fused"], want["single"]), (n, kw, got, want)


def _sampling_refusals(env, phrase, enable):
    """dn_mlp_step_sampled and dn_step_sampled on an env with a model on: refused, in these words."""
    lib, n = env._lib, env.num_envs
    z4, z1, z13 = torch.zeros((n, 4), device=DEV), torch.zeros(n, device=DEV), torch.zeros((n, 13), device=DEV)
    zp = torch.zeros((n, 13), device=DEV)
    log_std = (C.c_float * 4)(0, 0, 0, 0)
    rc = lib.dn_mlp_step_sampled(env._handle, C.byref(_capi_module().DnMlpNet()), 1, zp.data_ptr(), 13, log_std, 1, 0, z4.data_ptr(), z1.data_ptr(),
                                 *env._ptrs[0], None, None, None, None, None)
    assert rc == INVALID and lib.dn_last_error().decode() == \
        "dn_mlp_step_sampled does not carry %s (%s); use dn_mlp_forward + dn_policy_sample + dn_step" % (phrase, enable)
    rc = lib.dn_step_sampled(env._handle, z4.data_ptr(), log_std, 1, 0, z4.data_ptr(), z1.data_ptr(), z13.data_ptr(), *env._ptrs[0][1:],
                             None, None, None, None, None)
    assert rc == INVALID and lib.dn_last_error().decode() == \
        "dn_step_sampled does not carry %s (%s); use dn_policy_sample + dn_step there" % (phrase, enable)


def test_an_enabled_model_forces_one_wave_bound_or_not(tmp_path):
    pkg = _pkg()
    _capi = _capi_module()
    n = 256
    exe = build_program(tmp_path)
    for which in ("privileged", "goal"):
        env = _env(pkg, n)
        lib, h = env._lib, env._handle
        want = run_program(exe, num_cus=env.num_cus, num_envs=n)
        assert _shapes(env) == (want["fused"], want["single"]) == (4, 3)      # four tiles on an MI355X: the multi-wave kernels
        if which == "privileged":
            _capi.check(lib.dn_enable_privileged(h, C.byref(_capi.DnPrivilegedConfig(1, 0))))
            rows, bind = torch.zeros((1, n, 52), device=DEV), lib.dn_bind_privileged
            phrase, enable = "the privileged observations", "dn_enable_privileged"
        else:
            _capi.check(lib.dn_enable_goal(h, C.byref(_capi.DnGoalConfig(0, 0))))
            rows, bind = torch.zeros((1, n, 8), device=DEV), lib.dn_bind_goal
            phrase, enable = "the goal observations", "dn_enable_goal"
        assert _shapes(env) == (1, 1), which
        a = torch.zeros((n, 4), device=DEV)
        assert lib.dn_step(h, a.data_ptr(), *env._ptrs[0], None, None, None, None, None) == 0, lib.dn_last_error()
        torch.cuda.synchronize()
        assert env.step_count == 1
        _sampling_refusals(env, phrase, enable)
        _capi.check(bind(h, rows.data_ptr(), None, 1))
        assert _shapes(env) == (1, 1), which
        _capi.check(bind(h, None, None, 0))
        assert _shapes(env) == (1, 1), which
        env.close()
    env = _env(pkg, n)
    assert _shapes(env) == (4, 3)
    cfg = _capi.DnDynamicsConfig((C.c_float * 2)(0.9, 1.1), (C.c_float * 2)(0.9, 1.1), (C.c_float * 2)(0.9, 1.1), (C.c_float * 2)(0.9, 1.1), 1, 0)
    _capi.check(env._lib.dn_enable_dynamics(env._handle, C.byref(cfg)))
    assert _shapes(env) == (1, 1)
    _sampling_refusals(env, "the randomised dynamics", "dn_enable_dynamics")
    env.close()


def test_the_merged_bodies_refuse_in_order_and_word_for_word():
    pkg = _pkg()
    _capi = _capi_module()
    n = 64
    env, clip = _env(pkg, n), _env(pkg, n, clip_rew=True)
    lib = env._lib
    z4, z8, z1, z13 = torch.zeros((n, 4), device=DEV), torch.zeros((n, 8), device=DEV), torch.zeros(n, device=DEV), torch.zeros((n, 16), device=DEV)
    log_std = (C.c_float * 4)(0, 0, 0, 0)

    def sampled(e, mean, obs):
        return lib.dn_step_sampled(e._handle, mean, log_std, 1, 0, z4.data_ptr(), z1.data_ptr(), obs, *e._ptrs[0][1:], None, None, None, None, None)

    def squashed(e, rows, obs):
        return lib.dn_step_squashed(e._handle, rows, 1, 0, z4.data_ptr(), z1.data_ptr(), obs, *e._ptrs[0][1:], None, None, None, None, None)

    plain_only = ("%s is built for the configuration without reward wrappers / extra physics terms / RPM actions / random spawn / zero damping; "
                  "use %s + dn_step there")
    for call, src, required, aligned, refused in (
            (sampled, z4, "mean, log_std, actions_out, log_prob_out, obs, reward, done, truncated and found_targets are required",
             "mean, actions_out and obs must be 16-byte aligned", plain_only % ("dn_step_sampled", "dn_policy_sample")),
            (squashed, z8, "mu_log_std, actions_out, obs, reward, done, truncated and found_targets are required",
             "mu_log_std, actions_out and obs must be 16-byte aligned", plain_only % ("dn_step_squashed", "dn_squashed_sample"))):
        # a null obs comes first: before the alignment of the other pointers, on an env the call refuses anyway
        for e, ptr in ((env, src.data_ptr()), (env, src.data_ptr() + 4), (clip, src.data_ptr() + 4)):
            assert call(e, ptr, None) == INVALID and lib.dn_last_error().decode() == required
        # then a misaligned obs: before the configuration
        for e in (env, clip):
            assert call(e, src.data_ptr(), z13.data_ptr() + 4) == INVALID and lib.dn_last_error().decode() == aligned
        assert call(clip, src.data_ptr(), z13.data_ptr()) == INVALID and lib.dn_last_error().decode() == refused
    torch.cuda.synchronize()
    assert env.step_count == 0 and clip.step_count == 0          # nothing was launched

    rows = torch.zeros((1, n, 52), device=DEV)
    _capi.check(lib.dn_enable_privileged(env._handle, C.byref(_capi.DnPrivilegedConfig(1, 0))))
    _capi.check(lib.dn_enable_goal(env._handle, C.byref(_capi.DnGoalConfig(0, 0))))
    for bind, name, enable in ((lib.dn_bind_privileged, "privileged", "dn_enable_privileged"), (lib.dn_bind_goal, "goal", "dn_enable_goal")):
        assert bind(None, rows.data_ptr(), None, 1) == INVALID and lib.dn_last_error().decode() == "env is required"
        assert bind(clip._handle, rows.data_ptr(), None, 1) == -5          # DN_ERR_BAD_STATE
        assert lib.dn_last_error().decode() == "the %s observations are not enabled (%s)" % (name, enable)
        assert bind(env._handle, None, rows.data_ptr(), 0) == INVALID        # before capacity_steps
        assert lib.dn_last_error().decode() == "terminal_rows without rows: rows = NULL unbinds both"
        for r, t in ((rows.data_ptr() + 4, None), (rows.data_ptr(), rows.data_ptr() + 4)):
            assert bind(env._handle, r, t, 0) == INVALID                     # before capacity_steps
            assert lib.dn_last_error().decode() == "rows and terminal_rows must be 16-byte aligned"
        assert bind(env._handle, rows.data_ptr(), None, 0) == INVALID
        assert lib.dn_last_error().decode() == "capacity_steps must be >= 1 (got 0)"
        _capi.check(bind(env._handle, rows.data_ptr(), rows.data_ptr(), 1))
        _capi.check(bind(env._handle, None, None, 0))
    env.close()
    clip.close()

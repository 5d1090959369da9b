"""``env.step`` as a differentiable function of the action, and the pyramid and Shack-Hartmann sensors as ones of the mirror command (``torch.autograd``)."""
from __future__ import annotations

import torch


class _StepOutputs(torch.autograd.Function):
    @staticmethod
    def forward(ctx, action, env):
        a = env._as_actions(action.detach())
        env.step(a)
        # the float64 outputs of the gradient's own forward half: what backward differentiates
        one = torch.ones(env.num_envs, dtype=torch.float64, device=env.device)
        _, vals = env.output_gradient(g_strehl=one, wrt=None, with_values=True)
        ctx.env = env
        ctx.epoch = env.state_epoch
        ctx.action = a
        ctx.in_dtype = action.dtype
        n = env.obs_dim ** 2
        return vals[:, :n].contiguous(), vals[:, n].contiguous(), vals[:, n + 1].contiguous()

    @staticmethod
    def backward(ctx, g_obs, g_power, g_strehl):
        env = ctx.env
        if env.state_epoch != ctx.epoch:
            raise RuntimeError("step_outputs: the environment has been stepped, reset or restored since this step; its gradient is that of the "
                               "state the step left and can only be taken before the state moves on")
        no_obs = env.obs_route == "separable" and not env.obs_gradient
        grad = env.output_gradient(g_obs=None if no_obs else g_obs, g_power=g_power, g_strehl=g_strehl, wrt="action", action=ctx.action)
        return grad.to(ctx.in_dtype), None


def step_outputs(env, action):
    """Step ``env`` (a ``BatchedAOEnv``) with ``action`` [B, A] and return ``(obs_raw [B, o^2], power [B], strehl [B])`` as float64 tensors
    that are differentiable with respect to ``action``.

    The forward pass is ``env.step(action)``; the values are the float64 ones ``output_gradient`` evaluates at that state (the step's own
    float32 outputs rounded from the same sums).  The backward pass is ONE ``env.output_gradient(wrt="action")`` call with the incoming
    cotangents.  The gradient is that of the state at this step: backward raises ``RuntimeError`` once the env has been stepped, reset or
    restored since, so call ``backward()`` (or ``torch.autograd.grad``) before the next step.

    One step is the whole chain here: the atmosphere never depends on the action, and a step sets the mirror absolutely from its action
    (AO_env.py:115-120), so nothing step t returns depends on an earlier action — the sum of per-step gradients is the exact policy
    gradient of an episode's return.  The Strehl reward (AO_env.py:476) is ``strehl`` itself; the SSIM reward (AO_env.py:487) is a function
    of ``obs_raw`` and ``power`` that callers write in torch and chain through these outputs.  On the separable observation route the
    observation has its gradient on envs made with ``obs_gradient=True``; without it ``obs_raw`` comes back as NaN and its cotangent is
    ignored, while power and Strehl keep theirs.

    Not on an env built with ``servo=`` (``RuntimeError``, before anything is stepped): there the mirror receives ``servo.apply(action)``,
    which depends on the earlier commands and on the mirror's state, so one step is no longer the whole chain and the derivative with
    respect to the command is not this call's to give (it is ``response (1 - f)`` of the applied action's at a latency below one frame,
    zero from one frame on, and earlier steps' gradients flow into later outputs).  ``env.step(action)`` followed by
    ``env.output_gradient(wrt="action")`` gives the gradient with respect to ``info["applied_action"]``, what the mirror received."""
    env._refuse_with_servo("step_outputs", 'env.step(action) and env.output_gradient(wrt="action"), the gradient with respect to info["applied_action"]',
                           why="the mirror receives servo.apply(action), which depends on earlier commands, so the one-step gradient with respect to "
                               "the command is not the derivative of what the step returns")
    obs_raw, power, strehl = _StepOutputs.apply(action, env)
    return obs_raw, power, strehl


class _PyramidOutput(torch.autograd.Function):
    @staticmethod
    def forward(ctx, actuators, env, which):
        a = actuators.detach().to(torch.float64).contiguous()
        frames, slopes = env.pyramid_clean(actuators=a)   # the gradient call's forward half alone
        ctx.env, ctx.epoch, ctx.act, ctx.which, ctx.in_dtype = env, env.state_epoch, a, which, actuators.dtype
        return slopes if which == "slopes" else frames

    @staticmethod
    def backward(ctx, g):
        env = ctx.env
        if env.state_epoch != ctx.epoch:
            raise RuntimeError("pyramid_" + ctx.which + ": the environment has been stepped, reset or restored since the forward pass; the "
                               "gradient is that of the state it saw and can only be taken before the state moves on")
        kw = {"g_slopes": g} if ctx.which == "slopes" else {"g_frames": g}
        return env.pyramid_gradient(actuators=ctx.act, **kw).to(ctx.in_dtype), None, None


def pyramid_slopes(env, actuators):
    """The clean slopes [B, 2 n_valid] (float64) of ``env``'s pyramid sensor with the mirror at ``actuators`` [B, A] (metres of surface, the
    units of ``get_actuators()``), differentiable with respect to ``actuators``.  The atmosphere is the state the last reset or step left;
    the mirror itself is not moved.  Forward is ``env.pyramid_clean``, backward one ``env.pyramid_gradient`` call; backward raises ``RuntimeError`` once
    the env has been stepped, reset or restored since.  Photon noise is not part of it."""
    return _PyramidOutput.apply(actuators, env, "slopes")


def pyramid_frames(env, actuators):
    """As ``pyramid_slopes``, for the clean frames [B, 4, n_s, n_s]."""
    return _PyramidOutput.apply(actuators, env, "frames")


class _ShackOutput(torch.autograd.Function):
    @staticmethod
    def forward(ctx, actuators, env, which):
        a = actuators.detach().to(torch.float64).contiguous()
        image, slopes = env.sh_clean(actuators=a)   # the gradient call's forward half alone
        ctx.env, ctx.epoch, ctx.act, ctx.which, ctx.in_dtype = env, env.state_epoch, a, which, actuators.dtype
        return slopes if which == "slopes" else image

    @staticmethod
    def backward(ctx, g):
        env = ctx.env
        if env.state_epoch != ctx.epoch:
            raise RuntimeError("sh_" + ctx.which + ": the environment has been stepped, reset or restored since the forward pass; the "
                               "gradient is that of the state it saw and can only be taken before the state moves on")
        kw = {"g_slopes": g} if ctx.which == "slopes" else {"g_image": g}
        return env.sh_gradient(actuators=ctx.act, **kw).to(ctx.in_dtype), None, None


def sh_slopes(env, actuators):
    """The clean slopes [B, 2 n_sub] (float64) of ``env``'s Shack-Hartmann sensor with its mirror at ``actuators`` [B, A] (metres of surface),
    differentiable with respect to ``actuators``.  The atmosphere is the state the last reset or step left; no mirror is moved.  Forward is
    ``env.sh_clean``, backward one ``env.sh_gradient`` call; backward raises ``RuntimeError`` once the env has been stepped, reset or
    restored since.  Photon noise is not part of it."""
    return _ShackOutput.apply(actuators, env, "slopes")


def sh_image(env, actuators):
    """As ``sh_slopes``, for the clean detector image [B, N*N]."""
    return _ShackOutput.apply(actuators, env, "image")

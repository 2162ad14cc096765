#!/usr/bin/env python3
"""Every output of the loss heads' entry points, bit for bit, for comparing two builds of the library (DN_LIB_PATH picks one):
    python3 profiles/loss_heads_outputs.py write OUT.npz        one build, in a fresh process each
    python3 profiles/loss_heads_outputs.py compare A.npz B.npz  exit status 0 when every array has the same bytes
The inputs are the data sets of tests/ppo_loss_support.py and tests/sac_loss_support.py at the tests' shapes: batch in BATCHES x act_dim in
ACT_DIMS (dn_ppo_loss with every spread, the value clip off and on and both coefficient pairs; dn_sac_policy and dn_sac_policy_backward)
and batch x n_critics in CRITICS (dn_sac_critic_loss with each gamma, dn_sac_actor_loss; a learned and a fixed coefficient).  What is
kept is every static output tensor of the four classes, stats included, as the integer view of its bytes."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def bits(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def write(target):
    import torch

    import drl_dronenavigation_amd as pkg
    import ppo_loss_support as P
    import sac_loss_support as S

    dev = torch.device("cuda:0")
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    out = {}

    def keep(tag, obj, names):
        torch.cuda.synchronize(dev)
        for name in names:
            out[f"{tag}/{name}"] = bits(getattr(obj, name))

    for batch in P.BATCHES:
        for act_dim in P.ACT_DIMS:
            for spread in P.SPREADS:
                d = {k: to(v) for k, v in P.data(batch, act_dim, spread).items()}
                mb = dict(actions=d["actions"], log_probs=d["old_log_prob"], advantages=d["advantages"], returns=d["returns"], values=d["old_values"])
                for value_clip in (False, True):
                    for ent_coef, vf_coef in P.COEFS:
                        ppo = pkg.PpoLoss(batch, act_dim, dev, clip_range=P.CLIP_RANGE, clip_range_vf=P.CLIP_RANGE_VF if value_clip else None,
                                          ent_coef=ent_coef, vf_coef=vf_coef)
                        ppo(d["mean"], d["log_std"], d["values"], mb)
                        keep(f"ppo/{batch}/{act_dim}/{spread}/{value_clip}/{ent_coef}", ppo, ("d_mean", "d_log_std", "d_value", "log_probs", "loss", "stats"))
            d = {k: to(v) for k, v in S.policy_data(batch, act_dim).items()}
            head = pkg.SacPolicyHead(batch, act_dim, dev)
            mean, log_std = d["mean"].clone().requires_grad_(), d["log_std"].clone().requires_grad_()
            actions, log_prob = head(mean, log_std, d["noise"])
            torch.autograd.backward([actions, log_prob], [d["g_actions"], d["g_log_prob"]])
            keep(f"policy/{batch}/{act_dim}", head, ("actions", "log_prob", "d_mean", "d_log_std"))
        for n_critics in S.CRITICS:
            d = {k: (tuple(to(x) for x in v) if isinstance(v, tuple) else to(v)) for k, v in S.loss_data(batch, n_critics).items()}
            for learned in (True, False):
                ent_coef = None if learned else S.FIXED_ENT_COEF
                for gamma in S.GAMMAS:
                    crit = pkg.SacCriticLoss(batch, dev, n_critics=n_critics, gamma=gamma, ent_coef=ent_coef)
                    crit(list(d["q"]), list(d["next_q"]), d["next_log_prob"], dict(rewards=d["rewards"], dones=d["dones"]),
                         d["log_ent_coef"] if learned else None)
                    keep(f"critic/{batch}/{n_critics}/{learned}/{gamma}", crit, ("d_q", "target_q", "loss", "stats"))
                act = pkg.SacActorLoss(batch, dev, n_critics=n_critics, target_entropy=S.TARGET_ENTROPY, ent_coef=ent_coef)
                act(d["log_prob"], list(d["q_pi"]), d["log_ent_coef"] if learned else None)
                keep(f"actor/{batch}/{n_critics}/{learned}", act, ("d_log_prob", "d_q_pi", "d_log_ent_coef", "actor_loss", "ent_coef_loss", "stats"))
    os.makedirs(os.path.dirname(os.path.abspath(target)), exist_ok=True)
    np.savez(target, **out)
    print(f"{len(out)} arrays, {sum(a.nbytes for a in out.values())} bytes -> {target} (library: {os.environ.get('DN_LIB_PATH', 'in-tree')})")


def compare(first, second):
    a, b = np.load(first), np.load(second)
    names = sorted(set(a.files) | set(b.files))
    differ = [n for n in names if n not in a.files or n not in b.files or not np.array_equal(a[n], b[n])]
    for n in differ:
        print("differs:", n)
    print(f"{len(names)} arrays, {len(differ)} differ")
    return 1 if differ or not names else 0


if __name__ == "__main__":
    sys.exit(write(sys.argv[2]) if sys.argv[1] == "write" else compare(sys.argv[2], sys.argv[3]))

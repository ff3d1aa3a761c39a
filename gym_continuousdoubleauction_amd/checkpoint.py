"""Resumable training runs: checkpoint directories and the learner-state records the fused loops save and restore.

The run surface of the reference (config/train_config.json "run": chkpt_freq, chkpt_keep, is_restore, restore_path, num_iters_is_delta): a checkpoint
is a directory `iter_<n>` (n = iterations completed, 1-based) under the run's checkpoint directory, written as `iter_<n>.tmp` and renamed when complete;
the newest `keep` are kept.  A restore takes the newest one (or a named one); the iteration count is then the TARGET, unless iters_is_delta.

A checkpoint holds everything the next iteration reads, so that a resumed run continues the same markets, RNG streams and episodes bit for bit:
    env.snap        the env's snapshot file (snapshot.save_snapshot: every market, spilled books included)
    state.pt        {"format", "version", "kind", "iteration", "run_id", "args"} + the learner: per trained net theta / adam_m / adam_v / adam_step,
                    the rollout chains' seed and counters, the update's shuffle seed and epoch count, the KL coefficient, the running episode returns
    league/         (league checkpoints) save_league's policy files of every bank row and its league.json
Everything here is host code; only the env snapshot needs the device."""
import os
import re
import shutil
import uuid

import torch

CHECKPOINT_FORMAT = "cda-train-checkpoint"
CHECKPOINT_VERSION = 1
STATE_FILE = "state.pt"
ENV_FILE = "env.snap"
LOOPS = {"ppo": "ppo.train_fused", "league": "league_train.train_league_fused"}        # checkpoint kind -> the loop that writes it
_NAME = re.compile(r"^iter_(\d+)$")


def checkpoint_name(n_done):
    return f"iter_{int(n_done)}"


def is_checkpoint(path):
    return os.path.isdir(path) and _NAME.match(os.path.basename(os.path.normpath(path))) is not None and os.path.isfile(os.path.join(path, STATE_FILE))


def list_checkpoints(checkpoint_dir):
    """[(n, path)] of the complete checkpoints under checkpoint_dir, oldest first (staging `.tmp` directories and anything else are skipped)"""
    if checkpoint_dir is None or not os.path.isdir(checkpoint_dir):
        return []
    out = []
    for name in os.listdir(checkpoint_dir):
        m = _NAME.match(name)
        path = os.path.join(checkpoint_dir, name)
        if m and is_checkpoint(path):
            out.append((int(m.group(1)), path))
    return sorted(out)


def newest_checkpoint(checkpoint_dir):
    cks = list_checkpoints(checkpoint_dir)
    return cks[-1][1] if cks else None


def resolve_restore(checkpoint_dir, restore):
    """restore=True: the newest checkpoint under checkpoint_dir (FileNotFoundError if there is none); a path: that checkpoint (ValueError if it is not one)"""
    if restore is True:
        path = newest_checkpoint(checkpoint_dir)
        if path is None:
            raise FileNotFoundError(f"restore=True but {checkpoint_dir!r} holds no checkpoint")
        return path
    path = os.fspath(restore)
    if not is_checkpoint(path):
        raise ValueError(f"{path!r} is not a checkpoint (an iter_<n> directory holding {STATE_FILE})")
    return path


def iteration_range(done, iters, iters_is_delta=False):
    """the iterations a run still runs (0-based global numbers): `iters` is the target count, or - iters_is_delta - the number of further iterations"""
    done = int(done)
    target = done + int(iters) if iters_is_delta else int(iters)
    return range(done, max(done, target))


def prune(checkpoint_dir, keep):
    """remove all but the newest `keep` checkpoints (keep <= 0 keeps all)"""
    if keep is None or int(keep) <= 0:
        return
    for _, path in list_checkpoints(checkpoint_dir)[:-int(keep)]:
        shutil.rmtree(path, ignore_errors=True)


def save_checkpoint(checkpoint_dir, n_done, state, env_snapshot=None, keep=3, extra_dirs=None):
    """write iter_<n_done> (staged as iter_<n_done>.tmp, renamed when complete), then prune to `keep`; returns its path.  extra_dirs {name: directory}:
    directories written beforehand (the league's policy files) that are moved into the checkpoint as <name>/"""
    from .snapshot import save_snapshot
    os.makedirs(checkpoint_dir, exist_ok=True)
    final = os.path.join(checkpoint_dir, checkpoint_name(n_done))
    tmp = final + ".tmp"
    shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(tmp)
    for name, src in (extra_dirs or {}).items():
        shutil.move(src, os.path.join(tmp, name))
    rec = dict(state, format=CHECKPOINT_FORMAT, version=CHECKPOINT_VERSION, iteration=int(n_done))
    torch.save(rec, os.path.join(tmp, STATE_FILE))
    if env_snapshot is not None:
        save_snapshot(os.path.join(tmp, ENV_FILE), env_snapshot)
    if os.path.exists(final):
        shutil.rmtree(final)
    os.rename(tmp, final)
    prune(checkpoint_dir, keep)
    return final


def check_state_record(rec):
    if not isinstance(rec, dict) or rec.get("format") != CHECKPOINT_FORMAT:
        raise ValueError(f"not a training checkpoint (format tag {rec.get('format') if isinstance(rec, dict) else type(rec).__name__!r}, want {CHECKPOINT_FORMAT!r})")
    if rec.get("version") != CHECKPOINT_VERSION:
        raise ValueError(f"checkpoint version {rec.get('version')!r} is not supported (this build reads version {CHECKPOINT_VERSION})")
    for k in ("kind", "iteration", "args", "run_id"):
        if k not in rec:
            raise ValueError(f"checkpoint record lacks {k!r}")
    return rec


def load_checkpoint(path):
    """(state dict, env Snapshot on the CPU or None) of a checkpoint directory; validated, no device needed"""
    from .snapshot import load_snapshot
    rec = check_state_record(torch.load(os.path.join(path, STATE_FILE), map_location="cpu", weights_only=True))
    env_path = os.path.join(path, ENV_FILE)
    return rec, (load_snapshot(env_path) if os.path.exists(env_path) else None)


def check_args(saved, now):
    """a resumed run must be the same run: every field of the saved loop arguments must equal the new one (ValueError naming the first that differs)"""
    for k in sorted(set(saved) | set(now)):
        if saved.get(k) != now.get(k):
            raise ValueError(f"checkpoint was written by a run with {k} = {saved.get(k)!r}, this run has {k} = {now.get(k)!r}")


def with_activation(args, activation):
    """the loop arguments of a run whose network has hidden activation `activation`: the "activation" key is added only when it is not tanh, so a tanh run's
    arguments are exactly what they were before the key existed (check_args compares the union of the keys: a tanh checkpoint written before then still
    resumes, and one of either kind refuses a run of the other)"""
    from .mlp import check_activation
    act = check_activation(activation)
    return dict(args, activation=act) if act != "tanh" else dict(args)


def with_vf_share_layers(args, vf_share_layers):
    """the loop arguments of a run with a shared-trunk network (RLlib's vf_share_layers): the "vf_share_layers" key is added only when it is True, so the arguments of a
    run with separate networks are exactly what they were before the key existed, and a checkpoint of either kind refuses a run of the other (check_args)"""
    return dict(args, vf_share_layers=True) if vf_share_layers else dict(args)


def with_scripted(args, profiles, trained_slots=None, scripted_weight=None):
    """the loop arguments of a run that trains against scripted opponents: the canonical fields of every profile, in order (scripted.profile_record), and
    trained_slots (ppo.train_fused) / scripted_weight (the league's pool weight).  Added only when there are scripted opponents: a run without them keeps the
    arguments it had before the keys existed, and check_args refuses a checkpoint of either kind for a run of the other, or one with other opponents"""
    from .scripted import profile_record
    profiles = list(profiles or [])
    if not profiles:
        return dict(args)
    out = dict(args, scripted_opponents=[profile_record(p) for p in profiles])
    if trained_slots is not None:
        out["trained_slots"] = int(trained_slots)
    if scripted_weight is not None:
        out["scripted_weight"] = float(scripted_weight)
    return out


def with_order_schedule(args, digest):
    """the loop arguments of a run on an env with an order schedule attached (CDAVecEnv.set_order_schedule): the schedule's digest (orders.schedule_digest) under
    "order_schedule".  Added only when a schedule is attached: a run without one keeps the arguments it had before the key existed, and check_args refuses a
    checkpoint written with another schedule, or with none, and the other way round"""
    return dict(args, order_schedule=str(digest)) if digest else dict(args)


def new_run_id():
    return uuid.uuid4().hex


# ---- learner-state records -------------------------------------------------------------------------------------------------------
def net_record(policy):
    """a FusedPolicy's trained state: theta and its Adam moments and step (CPU tensors)"""
    return {k: getattr(policy, k).detach().cpu().clone() for k in ("theta", "adam_m", "adam_v", "adam_step")}


def load_net_record(policy, rec):
    for k in ("theta", "adam_m", "adam_v", "adam_step"):
        dst, src = getattr(policy, k), rec[k]
        if tuple(dst.shape) != tuple(src.shape) or dst.dtype != src.dtype:
            raise ValueError(f"checkpoint {k} has shape {tuple(src.shape)} / {src.dtype}, the policy has {tuple(dst.shape)} / {dst.dtype}")
        dst.copy_(src)
    policy.pack()


def rollout_record(roll):
    return {"seed": int(roll.seed), "counters": roll._counters.detach().cpu().clone()}


def load_rollout_record(roll, rec):
    if int(rec["seed"]) != int(roll.seed):
        raise ValueError(f"checkpoint rollout seed {rec['seed']} != {roll.seed}")
    if tuple(rec["counters"].shape) != tuple(roll._counters.shape):
        raise ValueError(f"checkpoint has {rec['counters'].numel()} rollout chains, this run has {roll._counters.numel()}")
    roll._counters.copy_(rec["counters"])


def update_record(upd):
    return {"shuffle_seed": int(upd.shuffle_seed), "epochs_done": int(upd._epochs_done)}


def load_update_record(upd, rec):
    upd.shuffle_seed, upd._epochs_done = int(rec["shuffle_seed"]), int(rec["epochs_done"])


def returns_record(returns):
    """mlp.EpisodeReturns: the running return of every episode in progress (what history's episode_return of a later iteration adds to)"""
    return {"running": returns.running.detach().cpu().clone()}


def load_returns_record(returns, rec):
    if tuple(rec["running"].shape) != tuple(returns.running.shape):
        raise ValueError(f"checkpoint episode returns have shape {tuple(rec['running'].shape)}, this run has {tuple(returns.running.shape)}")
    returns.running.copy_(rec["running"])


def check_resumable(checkpoint_dir, chkpt_freq, restore, world=1, allreduce=None, recorder=None):
    """the refusals shared by both fused loops; returns whether the run is resumable (checkpoints written or a restore asked for)"""
    if int(chkpt_freq) < 0:
        raise ValueError("chkpt_freq must be >= 0")
    if int(chkpt_freq) > 0 and checkpoint_dir is None:
        raise ValueError("chkpt_freq > 0 needs a checkpoint_dir")
    resumable = checkpoint_dir is not None or bool(restore)
    if resumable and (world > 1 or allreduce is not None):
        raise ValueError("checkpoint / restore: data-parallel runs (world > 1) are not supported")
    if resumable and recorder is not None:
        raise ValueError("checkpoint / restore: an episode recorder's files cannot be resumed; run without a recorder")
    return resumable


# ---- the life cycle of a run ------------------------------------------------------------------------------------------------------
def run_args(policy, env, horizon, chains, objective, epochs, lr, minibatch, seed, episode_metrics):
    """the part of a checkpoint's `args` that both fused loops write (each adds its own keys), from a policy (the league: the bank's first), the env and the loop
    arguments.  Reads the policy's parameters on the host, so the loops build it for a resumable run only."""
    from .mlp import has_log_std_head, hidden_widths
    args = {"markets": int(env.n_markets), "agents": int(env.num_agents), "horizon": int(horizon), "chains": int(chains),
            "objective": {k: float(v) for k, v in objective.items()}, "hidden": [int(h) for h in hidden_widths(policy.theta)],
            "state_dependent_log_std": bool(has_log_std_head(policy.theta)), "epochs": int(epochs), "lr": float(lr), "minibatch": int(minibatch),
            "seed": int(seed), "episode_metrics": bool(episode_metrics)}
    return with_vf_share_layers(with_activation(args, policy.activation), getattr(policy, "vf_share_layers", False))


class Run:
    """One run of a fused loop (kind: a key of LOOPS), resumable or not: check_resumable's refusals (raised here), the checkpoint a restore continues (`state`, `snapshot`, `path`:
    None on a fresh run), the run id, the iterations to run (`its`) and the ones a checkpoint follows.  A resumable run calls open(args) once its argument record exists."""

    def __init__(self, kind, checkpoint_dir=None, chkpt_freq=0, chkpt_keep=3, restore=None, iters=0, iters_is_delta=False, world=1, allreduce=None, recorder=None, run_id=None):
        self.resumable = check_resumable(checkpoint_dir, chkpt_freq, restore, world=world, allreduce=allreduce, recorder=recorder)
        self.kind, self.checkpoint_dir, self.chkpt_freq, self.chkpt_keep, self.run_id = kind, checkpoint_dir, int(chkpt_freq), chkpt_keep, run_id
        self._restore, self._iters, self.its = restore, (iters, iters_is_delta), iteration_range(0, iters, iters_is_delta)
        self.args = self.path = self.state = self.snapshot = None

    def open(self, args):
        """args: the argument record.  A restore loads its checkpoint (ValueError: another loop's, or other arguments) and continues its run id and iteration count"""
        self.args, self.run_id = args, new_run_id() if self.run_id is None else self.run_id
        if self._restore:
            self.path = resolve_restore(self.checkpoint_dir, self._restore)
            self.state, self.snapshot = load_checkpoint(self.path)
            if self.state["kind"] != self.kind:
                raise ValueError(f"{self.path} is a {self.state['kind']!r} checkpoint, not a {LOOPS[self.kind]} one")
            check_args(self.state["args"], args)
            self.run_id, self.its = self.state["run_id"], iteration_range(self.state["iteration"], *self._iters)

    def start_env(self, env, seed, first_market, episode_metrics):
        """the env as the first iteration finds it: the checkpoint's markets on a restore, else reset with the seed of its first (global) market; its episode metrics
        in the state the loop was asked for, BOTH ways - an env that comes with them on runs an episode_metrics=False loop with them off (nothing would collect the
        accumulators), and the rollout graphs are captured after this"""
        def set_metrics():
            if episode_metrics:
                env.enable_episode_metrics(True)
            elif bool(getattr(env, "episode_metrics_on", False)):
                env.enable_episode_metrics(False)
        if self.state is not None:
            set_metrics()                                           # (before the restore: the snapshot carries the metrics setting and the running tallies)
            env.restore(self.snapshot)
        else:
            env.reset(seed=seed + int(first_market))
            set_metrics()

    def save(self, n_done, state, env, extra_dirs=None):
        """checkpoint_dir/iter_<n_done>: the loop's `state` under this run's kind, id and arguments, and the env's markets"""
        state = dict({"kind": self.kind, "run_id": self.run_id, "args": self.args}, **state)
        return save_checkpoint(self.checkpoint_dir, n_done, state, env.snapshot(), keep=self.chkpt_keep, extra_dirs=extra_dirs)

    def after_iteration(self, it, save, may_save=None):
        """save(n_done) after every chkpt_freq-th iteration, and after the run's last one where may_save(n_done) allows (None: anywhere; the league: at an episode boundary)"""
        due = self.chkpt_freq > 0 and (it + 1) % self.chkpt_freq == 0
        final = it == self.its[-1] and (may_save is None or may_save(it + 1))
        if self.checkpoint_dir is not None and (due or final):
            save(it + 1)

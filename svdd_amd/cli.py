"""Command-line decode drivers — the caller contract of the reference's `decode.py`,
`decode_tweedie.py`, `decode_TDS.py`, `decode_DPS.py`, `decode_classfier.py` (reference decode.py:52-211): seed, build the
nets, run `BaseModel.controlled_decode*`, write `./log/{task}-{reward_name}[_tw|_TDS|_DPS].npz` with
the two arrays `decoding` and `baseline` (decode.py:117, decode_tweedie.py:118, decode_TDS.py:118,
decode_DPS.py:119, decode_classfier.py:119).

Offline there are no W&B artifacts, so nets are random-init unless state_dicts are given
(`--diffusion_ckpt`, `--load_checkpoint_path`, `--reward_ckpt`; reference key names load unchanged).
Only the flags that reach the decode path are kept; the reference's ~40 vestigial training flags are not."""
import argparse
import os
import random

import numpy as np
import torch

SUFFIX = {"mc": "", "tweedie": "_tw", "tds": "_TDS", "dps": "_DPS", "classfier": "-classfier"}
GUIDANCE_DEFAULT = {"dps": 1e5, "classfier": 1.5}                                   # decode_DPS.py:184, decode_classfier.py


def set_seed(seed):
    """reference decode.py:31-35"""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)


def build_parser(method="mc"):
    p = argparse.ArgumentParser(description=f"SVDD decode ({method}) on MI355X")
    p.add_argument("--task", default="dna", choices=["dna", "rna"])                 # decode.py:130
    p.add_argument("--reward_name", default=None, help="HepG2 (dna) / MRL (rna) by default")
    p.add_argument("--batch_size", type=int, default=256)                            # :163
    p.add_argument("--sample_M", type=int, default=10)                               # :165
    p.add_argument("--val_batch_num", type=int, default=1)                           # :167
    p.add_argument("--seed", type=int, default=44)                                   # :181
    p.add_argument("--method", default=method, choices=list(SUFFIX))
    p.add_argument("--tweedie", default="True", help='"True": posterior-mean scoring (decode_tweedie.py:206)')
    p.add_argument("--alpha", type=float, default=0.5)                               # decode_TDS.py:183
    p.add_argument("--guidance_scale", type=float, default=None,
                   help="guidance scale of --method dps (default 1e5) and classfier (default 1.5)")
    p.add_argument("--model", default="convgru", choices=["convgru", "enformer"],
                   help="value-function trunk: convgru = ConvGRUTrunk + ConvHead (Enformer.py:32-49; BASELINE configs 1-3, SURVEY "
                        "section 8d); enformer = the 230 M-parameter EnformerTrunk(7, 1536, 11, 8, 64) + ConvHead(1, 3072) the "
                        "reference's decode.py:78-80 builds for --model enformer (BASELINE configs[3])")                   # decode.py:149
    p.add_argument("--precision", default="f32", choices=["f32", "f16x3", "bf16x3", "f16", "bf16"],
                   help="f32: exact fp32 net kernels (default, the parity reference); x3: fp32 operands split hi + lo on the 16-bit "
                        "matrix cores (f16x3: fp32-class error; bf16x3: a 16-bit operand, 1e-5-class); f16 / bf16: one pass. With --model enformer any non-f32 mode runs the "
                        "hand-written trunk kernels (bf16x3 / bf16); f32 runs the PyTorch module")
    p.add_argument("--rng", default="replay", choices=["replay", "philox"],
                   help="replay: the reference's torch-CPU RNG stream; philox: in-kernel counter RNG")
    p.add_argument("--diffusion_ckpt", default=None)
    p.add_argument("--load_checkpoint_path", default=None, help="value-function checkpoint ('model_state_dict')")
    p.add_argument("--reward_ckpt", default=None)
    p.add_argument("--out_dir", default="./log")
    p.add_argument("--eval_nll", type=int, default=0, metavar="K",
                   help="K > 0: also score the decoded and the baseline sequences by the pretrained model's ELBO (K draws per "
                        "sequence, nats): npz keys decoding_nll / baseline_nll")
    p.add_argument("--eval_quality", default=argparse.SUPPRESS, metavar="FILE.npz",      # absent unless given: without it the namespace is unchanged
                   help="also report the set-level quality of the decoded sequences (k-mer Pearson r, diversity, novelty, score "
                        "Wasserstein distance) against the token arrays train / valid / test of FILE.npz (any subset): printed, and "
                        "saved as npz keys quality_<metric>")
    p.add_argument("--eval_motifs", default=argparse.SUPPRESS, metavar="FILE.meme",      # absent unless given, as --eval_quality
                   help="with --eval_quality FILE.npz: also scan the decoded sequences for the motifs of FILE.meme (MEME text, as "
                        "JASPAR and HOCOMOCO are distributed) and report the Spearman correlation of their motif frequencies with "
                        "each reference set's, the mean number of hits per design and the number of reachable motifs: printed, and "
                        "saved as npz keys quality_<metric>")
    p.add_argument("--eval_edit", type=int, default=argparse.SUPPRESS, metavar="K",      # absent unless given, as --eval_quality
                   help="with --eval_quality FILE.npz: also report the near copies by edit distance (substitutions, insertions and "
                        "deletions), which the Hamming novelty cannot see: the share of designs with another design, and with a row "
                        "of `train`, within K edits, the smallest such distance, and the share the Hamming report misses: printed, "
                        "and saved as npz keys quality_<metric>")
    p.add_argument("--select", type=int, default=argparse.SUPPRESS, metavar="K",         # the four --select* flags: absent unless given
                   help="also choose a library of the K best decoded sequences that are no near copies of each other: walk them "
                        "from the highest reward prediction down and keep one when it is at least --select_min_dist substitutions "
                        "from every sequence kept: one line printed, and saved as npz keys selected (tokens), selected_idx, "
                        "selected_scores and library_<metric>")
    p.add_argument("--select_min_dist", type=int, default=argparse.SUPPRESS, metavar="D",
                   help="with --select: the smallest Hamming distance between two sequences of the library (default 1: no exact "
                        "duplicates)")
    p.add_argument("--select_revcomp", action="store_true", default=argparse.SUPPRESS,
                   help="with --select: a sequence is also a near copy of another's reverse complement")
    p.add_argument("--select_metric", choices=("hamming", "edit"), default=argparse.SUPPRESS,
                   help="with --select: what --select_min_dist counts. hamming (the default): substitutions. edit: substitutions, "
                        "insertions and deletions, so that a sequence and its copy shifted by a few bases are near copies too; the "
                        "same npz keys, and library_metric")
    p.add_argument("--guide_motifs", default=argparse.SUPPRESS, metavar="FILE.meme",     # the three --guide_* flags: absent unless given
                   help="--method tweedie only: decode towards (or away from) the motifs of FILE.meme, the reward net's score plus "
                        "a motif term (svdd_amd.motifs.MotifReward); give --guide_weights, --guide_margin or both")
    p.add_argument("--guide_weights", default=argparse.SUPPRESS, metavar="NAME=+2,NAME2=-1",
                   help="with --guide_motifs: the reward of a hit of motif NAME (negative: a penalty), counted once per design")
    p.add_argument("--guide_margin", default=argparse.SUPPRESS, metavar="NAME=0.01",
                   help="with --guide_motifs: the reward per score unit by which a design's best window of motif NAME falls short "
                        "of the motif's threshold (the dense signal that lets the decode climb towards a site)")
    p.add_argument("--presample", action="store_true",
                   help="pre-sample val_batch_num batches at construction like the reference's BaseModel.__init__")
    p.epilog = ("--method classfier evaluates the value net in eval mode for every task (the reference's decode_classfier.py leaves it in "
                "train mode for --task rna: dropout on, batch-statistics BatchNorm, an irreproducible run).")
    return p


def _guidance_scale(args):
    return args.guidance_scale if args.guidance_scale is not None else GUIDANCE_DEFAULT.get(args.method, 1e5)


_MOTIFS_NEED_SETS = "--eval_motifs needs --eval_quality FILE.npz: the reference sets its correlations are taken against"
_EDIT_NEEDS_SETS = "--eval_edit needs --eval_quality FILE.npz: the training set its near copies are looked for in"
_SELECT_NEEDS_K = "--{} needs --select K: the size of the library it shapes"


def _eval_error(args):
    """What is wrong with the --eval_* and --select* flags of args, or None."""
    if not hasattr(args, "select"):
        for flag in ("select_min_dist", "select_revcomp", "select_metric"):
            if hasattr(args, flag):
                return _SELECT_NEEDS_K.format(flag)
    if getattr(args, "eval_quality", None):
        return None
    return _MOTIFS_NEED_SETS if hasattr(args, "eval_motifs") else _EDIT_NEEDS_SETS if hasattr(args, "eval_edit") else None


_GUIDE_FLAGS = ("guide_motifs", "guide_weights", "guide_margin")


def _guide_error(args):
    """What is wrong with the --guide_* flags of args, or None."""
    given = [f for f in _GUIDE_FLAGS if hasattr(args, f)]
    if not given:
        return None
    if args.method != "tweedie":
        return f"--{given[0]} is for --method tweedie (SVDD-PM scores finished sequences), not --method {args.method}"
    if "guide_motifs" not in given:
        return f"--{given[0]} needs --guide_motifs FILE.meme"
    if len(given) == 1:
        return "--guide_motifs needs --guide_weights, --guide_margin or both"
    return None


def _name_values(text, flag):
    """"NAME=+2,NAME2=-1" -> {"NAME": 2.0, "NAME2": -1.0}."""
    out = {}
    for item in filter(None, (s.strip() for s in text.split(","))):
        name, eq, value = item.rpartition("=")
        try:
            number = float(value) if eq and name.strip() else None
        except ValueError:
            number = None
        if number is None:
            raise ValueError(f"--{flag}: expected NAME=NUMBER[,NAME=NUMBER ...], got {item!r}")
        out[name.strip()] = number
    if not out:
        raise ValueError(f"--{flag}: expected NAME=NUMBER[,NAME=NUMBER ...], got {text!r}")
    return out


def guide_reward(args):
    """The MotifReward of the --guide_* flags, or None."""
    if not hasattr(args, "guide_motifs"):
        return None
    from .motifs import MotifReward, load_meme
    return MotifReward(load_meme(args.guide_motifs),
                       hit_weight=_name_values(args.guide_weights, "guide_weights") if hasattr(args, "guide_weights") else None,
                       margin_weight=_name_values(args.guide_margin, "guide_margin") if hasattr(args, "guide_margin") else None)


def run(args):
    if _eval_error(args):
        raise ValueError(_eval_error(args))                     # before any model is built
    if _guide_error(args):
        raise ValueError(_guide_error(args))                    # so are these
    guide = guide_reward(args)                                  # ... and a file or a weight that does not parse
    from . import synthetic
    from .harness import BaseModel
    from .value_nets import load_reference_state_dict

    set_seed(args.seed)
    reward_name = args.reward_name or ("HepG2" if args.task == "dna" else "MRL")
    ref_model, embedding, head, reward = synthetic.build(args.task, "cuda", seed=args.seed, value=args.model)
    ref_model.precision = args.precision
    if args.diffusion_ckpt:
        sd = torch.load(args.diffusion_ckpt, map_location="cpu")
        ref_model.load_state_dict(sd.get("state_dict", sd), strict=False)
    if args.load_checkpoint_path:
        sd = torch.load(args.load_checkpoint_path, map_location="cpu")["model_state_dict"]
        emb_sd = {k[len("embedding."):]: v for k, v in sd.items() if k.startswith("embedding.")}
        if args.model == "enformer":                       # the reference's wrapper names -> this module's (enformer_value.py)
            from .enformer_value import load_reference_state_dict as load_trunk
            load_trunk(embedding, emb_sd)
        else:
            load_reference_state_dict(embedding, emb_sd)
        load_reference_state_dict(head, {k[len("head."):]: v for k, v in sd.items() if k.startswith("head.")})
    if args.reward_ckpt:
        sd = torch.load(args.reward_ckpt, map_location="cpu")
        load_reference_state_dict(reward, sd.get("model_state_dict", sd))
    ref_model.rng_mode, ref_model.philox_seed = args.rng, args.seed
    model = BaseModel(embedding, head, ref_model, reward, args.batch_size, task=args.task,
                      val_batch_num=args.val_batch_num if args.presample else 0).cuda().eval()
    if args.method == "mc":
        out = model.controlled_decode(gen_batch_num=args.val_batch_num, sample_M=args.sample_M)
    elif args.method == "tweedie" and guide is not None:
        out = model.controlled_decode_motif(gen_batch_num=args.val_batch_num, sample_M=args.sample_M, motif_reward=guide,
                                            options=args.tweedie)
        terms = torch.cat(model.motif_terms)
        print(f"motif term of the guided designs: mean {terms.mean().item():.4f} (n={terms.numel()})")
    elif args.method == "tweedie":
        out = model.controlled_decode_tweedie(gen_batch_num=args.val_batch_num, sample_M=args.sample_M, options=args.tweedie)
    elif args.method == "tds":
        out = model.controlled_decode_TDS(gen_batch_num=args.val_batch_num, sample_M=args.sample_M, alpha=args.alpha)
    elif args.method == "dps":
        out = model.controlled_decode_DPS(gen_batch_num=args.val_batch_num, sample_M=args.sample_M,
                                          guidance_scale=_guidance_scale(args))
    else:
        out = model.controlled_decode_classfier(gen_batch_num=args.val_batch_num, guidance_scale=_guidance_scale(args),
                                                sample_M=args.sample_M)
    gen_samples, value_func_preds, reward_model_preds, selected_baseline_preds, baseline_preds = out
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, f"{args.task}-{reward_name}{SUFFIX[args.method]}")
    extra, nll_note = {}, ""
    if args.eval_nll > 0:
        extra = dict(decoding_nll=model.evaluate_nll(gen_samples, args.eval_nll).cpu().numpy(),
                     baseline_nll=model.evaluate_nll(model.baseline_samples, args.eval_nll).cpu().numpy())
        nll_note = f", nll decoding {extra['decoding_nll'].mean():.4f} baseline {extra['baseline_nll'].mean():.4f} nats"
    report = None
    if getattr(args, "eval_quality", None):
        with np.load(args.eval_quality) as f:
            sets = {name: f[name] for name in ("train", "valid", "test") if name in f.files}
        report = model.evaluate_quality(gen_samples, refs=sets, train=sets.get("train"))
        if getattr(args, "eval_motifs", None):
            from .motifs import load_meme
            report.update(model.evaluate_motifs(gen_samples, load_meme(args.eval_motifs), refs=sets))
        if hasattr(args, "eval_edit"):
            report.update(model.evaluate_edit(gen_samples, args.eval_edit, train=sets.get("train")))
        extra.update({f"quality_{key}": np.float64(v) for key, v in report.items()})
    library = None
    if hasattr(args, "select"):
        edit = getattr(args, "select_metric", "hamming") == "edit"
        tokens, scores, idx, library = (model.select_library_edit if edit else model.select_library)(
            gen_samples, args.select, getattr(args, "select_min_dist", 1), revcomp=getattr(args, "select_revcomp", False))
        extra.update(selected=tokens.cpu().numpy(), selected_idx=idx.cpu().numpy(), selected_scores=scores.cpu().numpy())
        if edit:
            extra.update(library_metric=np.str_("edit"))
        extra.update({key if key.startswith("library_") else f"library_{key}": np.float64(v) for key, v in library.items()})
    np.savez(path, decoding=reward_model_preds.cpu().numpy(), baseline=baseline_preds.cpu().numpy(), **extra)
    print(f"wrote {path}.npz: decoding mean {reward_model_preds.mean().item():.4f} (n={reward_model_preds.numel()}), "
          f"baseline mean {baseline_preds.mean().item():.4f}{nll_note}")
    if library is not None:
        print("library: " + ", ".join(f"{key} {v:.4f}" for key, v in library.items()))
    if report is not None:
        print("quality: " + ", ".join(f"{key} {v:.4f}" for key, v in report.items()))
    return path + ".npz", out


def main(method="mc", argv=None):
    parser = build_parser(method)
    args = parser.parse_args(argv)
    if _eval_error(args):
        parser.error(_eval_error(args))
    if _guide_error(args):
        parser.error(_guide_error(args))
    return run(args)


# ------------------------------------------------------------------ value-function training (train_value.py) ----
def build_train_parser():
    p = argparse.ArgumentParser(description="Train the SVDD value function on MI355X: Monte-Carlo regression or CD-Q "
                                            "(reference Enformer.BaseModel.forward, Enformer.py:163-267)")
    p.add_argument("--task", default="dna", choices=["dna", "rna"])
    p.add_argument("--cdq", action="store_true", help="CD-Q: regress every state onto the value net's own mean over 10 next states "
                                                      "(default: Monte-Carlo regression onto r(x_0))")
    p.add_argument("--cdq_alpha", type=float, default=None,
                   help="CD-Q with the soft backup alpha log mean exp(v / alpha) instead of the reference's mean")
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--batch_size", type=int, default=256)
    p.add_argument("--steps", type=int, default=None, help="diffusion steps of a rollout (default: the task's config, 128)")
    p.add_argument("--seed", type=int, default=44)
    p.add_argument("--rng", default="philox", choices=["replay", "philox"])
    p.add_argument("--out", default="./log/value_net.pt", help="where the value net's state_dict is saved ('model_state_dict', the "
                                                               "layout --load_checkpoint_path of the decode scripts reads)")
    return p


def train_value(args):
    """N AdamW iterations of BaseModel.forward on the synthetic nets -> (path of the saved state_dict, losses). Every iteration
    builds its training set with one rollout on the device (Diffusion.value_targets) and takes one optimiser step on it."""
    from . import synthetic
    from .harness import BaseModel

    set_seed(args.seed)
    ref_model, embedding, head, reward = synthetic.build(args.task, "cuda", seed=args.seed)
    if args.steps is not None:
        ref_model.config.sampling.steps = args.steps
    ref_model.rng_mode, ref_model.philox_seed = args.rng, args.seed
    for p in list(embedding.parameters()) + list(head.parameters()):
        p.requires_grad_(True)
    model = BaseModel(embedding, head, ref_model, reward, args.batch_size, task=args.task, cdq=args.cdq or args.cdq_alpha is not None,
                      cdq_alpha=args.cdq_alpha).cuda().train()
    opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=args.lr)
    losses = []
    for it in range(args.iters):
        ref_model.philox_seed = args.seed + it                # Philox: a rollout is a function of the key; replay draws on
        opt.zero_grad(set_to_none=True)
        loss = model()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        print(f"iter {it}: loss {losses[-1]:.6f}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    sd = {f"embedding.{k}": v for k, v in embedding.state_dict().items()}
    sd.update({f"head.{k}": v for k, v in head.state_dict().items()})
    torch.save({"model_state_dict": sd}, args.out)
    print(f"wrote {args.out}")
    return args.out, losses


def main_train(argv=None):
    return train_value(build_train_parser().parse_args(argv))


if __name__ == "__main__":
    main()

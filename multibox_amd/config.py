"""config.yaml loader -- same keys as the reference (config.py:6-12, config.yaml.example:1-151),
attribute access like its EasyDict (easydict itself is not installed here)."""
import ctypes

import yaml


class Cfg(dict):
    """Minimal EasyDict stand-in: nested dicts become attribute-accessible."""

    def __init__(self, d=None):
        super().__init__()
        for k, v in (d or {}).items():
            self[k] = v

    def __setitem__(self, k, v):
        if isinstance(v, dict) and not isinstance(v, Cfg):
            v = Cfg(v)
        elif isinstance(v, list):
            v = [Cfg(x) if isinstance(x, dict) else x for x in v]
        super().__setitem__(k, v)

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    __setattr__ = __setitem__


DEFAULTS = dict(NUM_BBOXES_PER_CELL=5, MAX_NUM_BBOXES=13, LOCATION_LOSS_ALPHA=1000.0, BATCH_SIZE=32, INPUT_SIZE=299,
                NUM_TRAIN_EXAMPLES=56945, NUM_TRAIN_ITERATIONS=1000000, INITIAL_LEARNING_RATE=0.01, NUM_EPOCHS_PER_DELAY=4,
                LEARNING_RATE_DECAY_FACTOR=0.94, LEARNING_RATE_STAIRCASE=True, RMSPROP_DECAY=0.9, RMSPROP_MOMENTUM=0,
                RMSPROP_EPSILON=1.0, BATCHNORM_MOVING_AVERAGE_DECAY=0.9997, MOVING_AVERAGE_DECAY=0.9999,
                LOG_EVERY_N_STEPS=10, SAVE_INTERVAL_SECS=3600, MAX_TO_KEEP=3)


def parse_config_file(path_to_config):
    """config.py:6-12 (safe_load instead of the reference's Loader-less yaml.load)."""
    with open(path_to_config) as f:
        cfg = yaml.safe_load(f)
    return Cfg(cfg)


def with_defaults(cfg):
    out = Cfg(DEFAULTS)
    for k, v in cfg.items():
        out[k] = v
    return out


def _int_key(cfg, key, minimum):
    """cfg[key] as an int >= minimum.  A float without a fraction counts (3.0); a bool, a float with a fraction, a string
    or anything else raises ValueError naming the key."""
    v = cfg[key]
    ok = isinstance(v, (int, float)) and not isinstance(v, bool) and minimum <= v <= 2 ** 31 - 1 and v == int(v)
    if not ok:
        raise ValueError("%s must be an integer in [%d, 2^31), got %r" % (key, minimum, v))
    return int(v)


def negative_mining(cfg):
    """Hard-negative mining for the confidence loss (mbx_loss_fwd_bwd_mined; not in the reference, so off when absent):
    None, or (neg_per_pos, min_neg) from LOSS_NEG_PER_POS (an int >= 1; absent or null = off) and LOSS_MIN_NEG (an int
    >= 0, default 0; only with LOSS_NEG_PER_POS).  Per image the max(min_neg, neg_per_pos * positives) highest-scoring
    negatives are kept.  Raises ValueError naming the key.  Host code only."""
    if cfg.get("LOSS_NEG_PER_POS") is None:
        if cfg.get("LOSS_MIN_NEG") is not None:
            raise ValueError("LOSS_MIN_NEG is given without LOSS_NEG_PER_POS")
        return None
    neg_per_pos = _int_key(cfg, "LOSS_NEG_PER_POS", 1)
    return neg_per_pos, (_int_key(cfg, "LOSS_MIN_NEG", 0) if cfg.get("LOSS_MIN_NEG") is not None else 0)


def match_iou_threshold(cfg):
    """Threshold matching behind the bipartite match (mbx_match_extend; not in the reference, so off when absent): None,
    or LOSS_MATCH_IOU_THRESHOLD as a float in (0, 1] (absent or null = off).  Every prior the bipartite match left free
    goes to the box it overlaps most if that IoU is over the key.  A bool, a string, a list, a NaN or a value outside
    (0, 1] raises ValueError naming the key.  Host code only."""
    v = cfg.get("LOSS_MATCH_IOU_THRESHOLD")
    if v is None:
        return None
    if not (isinstance(v, (int, float)) and not isinstance(v, bool) and 0 < v <= 1):
        raise ValueError("LOSS_MATCH_IOU_THRESHOLD must be a number in (0, 1], got %r" % (v,))
    return float(v)


def atss_matching(cfg):
    """ATSS matching behind the bipartite match (mbx_match_atss; not in the reference, so off when absent): None, or
    LOSS_MATCH_ATSS_TOPK as an int >= 1 (absent or null = off).  Per box the key's number of priors nearest to its centre on
    every pyramid level are candidates, and the free ones at or over the mean plus the standard deviation of the
    candidates' IoUs, with their centre in the box, become its positives.  With NUM_BBOXES_PER_CELL priors sharing a centre,
    9 reaches about two cells of a level; the paper's nine locations are 9 * NUM_BBOXES_PER_CELL.  Not together with
    LOSS_MATCH_IOU_THRESHOLD (both decide what a free prior becomes): ValueError naming both keys.  A bool, a float with a
    fraction, a string, a list, a NaN or a value < 1 raises ValueError naming the key.  Host code only."""
    if cfg.get("LOSS_MATCH_ATSS_TOPK") is None:
        return None
    topk = _int_key(cfg, "LOSS_MATCH_ATSS_TOPK", 1)
    if cfg.get("LOSS_MATCH_IOU_THRESHOLD") is not None:
        raise ValueError("LOSS_MATCH_ATSS_TOPK and LOSS_MATCH_IOU_THRESHOLD are both given: choose one matching rule")
    return topk


def tal_matching(cfg):
    """Task-aligned matching behind the bipartite match (mbx_match_tal, TOOD's assigner; not in the reference, so off when
    absent): None, or the Trainer's keyword arguments {tal_topk, tal_alpha, tal_beta} from
      LOSS_MATCH_TAL_TOPK   an int >= 1 (13 in the paper); absent or null = off.  Per box the key's number of priors with
                            their centre inside it whose prediction scores the largest conf^alpha * IoU^beta are selected,
                            and the free ones become positives of the box their prediction overlaps most.
      LOSS_MATCH_TAL_ALPHA  a multiple of 0.5 in [0, 4], default 1.0; only with the first.
      LOSS_MATCH_TAL_BETA   an int in [1, 16], default 6; only with the first.
    Not together with LOSS_MATCH_IOU_THRESHOLD or LOSS_MATCH_ATSS_TOPK (each decides what a free prior becomes): ValueError
    naming both keys.  A bool, a string, a list, a NaN or a value out of range raises ValueError naming the key.  Host code
    only."""
    if cfg.get("LOSS_MATCH_TAL_TOPK") is None:
        for key in ("LOSS_MATCH_TAL_ALPHA", "LOSS_MATCH_TAL_BETA"):
            if cfg.get(key) is not None:
                raise ValueError("%s is given without LOSS_MATCH_TAL_TOPK" % key)
        return None
    topk = _int_key(cfg, "LOSS_MATCH_TAL_TOPK", 1)
    for key in ("LOSS_MATCH_IOU_THRESHOLD", "LOSS_MATCH_ATSS_TOPK"):
        if cfg.get(key) is not None:
            raise ValueError("LOSS_MATCH_TAL_TOPK and %s are both given: choose one matching rule" % key)
    alpha = cfg.get("LOSS_MATCH_TAL_ALPHA")
    if alpha is None:
        alpha = 1.0
    elif not (isinstance(alpha, (int, float)) and not isinstance(alpha, bool) and 0 <= alpha <= 4 and alpha * 2 == int(alpha * 2)):
        raise ValueError("LOSS_MATCH_TAL_ALPHA must be a multiple of 0.5 in [0, 4], got %r" % (alpha,))
    beta = 6
    if cfg.get("LOSS_MATCH_TAL_BETA") is not None:
        beta = _int_key(cfg, "LOSS_MATCH_TAL_BETA", 1)
        if beta > 16:
            raise ValueError("LOSS_MATCH_TAL_BETA must be an integer in [1, 16], got %r" % (beta,))
    return {"tal_topk": topk, "tal_alpha": float(alpha), "tal_beta": beta}


def focal_loss(cfg):
    """Focal loss on the confidence term (mbx_loss_fwd_bwd_focal; not in the reference, so off when absent): None, or
    (gamma, alpha_or_None) from LOSS_FOCAL_GAMMA (a number in [0, 10]; absent or null = off) and LOSS_FOCAL_ALPHA (a number
    strictly inside (0, 1), default null = both sides weigh 1; only with LOSS_FOCAL_GAMMA).  Alpha weighs the positives and
    1 - alpha the negatives, the paper's convention (0.25 with gamma = 2).  A bool, a string, a list, a NaN or a value
    out of range raises ValueError naming the key.  Host code only."""
    number = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool)
    gamma, alpha = cfg.get("LOSS_FOCAL_GAMMA"), cfg.get("LOSS_FOCAL_ALPHA")
    if gamma is None:
        if alpha is not None:
            raise ValueError("LOSS_FOCAL_ALPHA is given without LOSS_FOCAL_GAMMA")
        return None
    if not (number(gamma) and 0 <= gamma <= 10):
        raise ValueError("LOSS_FOCAL_GAMMA must be a number in [0, 10], got %r" % (gamma,))
    if alpha is not None and not (number(alpha) and 0 < alpha < 1):
        raise ValueError("LOSS_FOCAL_ALPHA must be a number inside (0, 1), got %r" % (alpha,))
    return float(gamma), (None if alpha is None else float(alpha))


LOC_LOSS_TYPES = ("l2", "smooth_l1", "giou", "diou", "ciou")      # MBX_LOC_L2 = 0 .. MBX_LOC_CIOU = 4 (include/mbx.h)


def loc_loss(cfg):
    """The location term of a positive (mbx_loss_fwd_bwd_loc; the reference has L2 alone, so off when absent): None, or
    (type, beta_or_None) from LOSS_LOC_TYPE (one of l2, smooth_l1, giou, diou, ciou; absent or null = off, the reference's
    L2 through the entry the other keys choose) and LOSS_LOC_BETA (a number that is finite and > 0 as a float32, default
    0.1; only with smooth_l1, where it is the residual at which the term turns from quadratic to linear -- beta is None
    for every other type).  The match keeps the reference's L2-based cost.  LOCATION_LOSS_ALPHA's default of 1000 was
    sized for L2: with giou, diou or ciou, whose term is of order 1 per positive, set your own.  A value that is no such
    string, a bool, a list, a NaN, an infinity or a beta <= 0 raises ValueError naming the key.  Host code only."""
    kind, beta = cfg.get("LOSS_LOC_TYPE"), cfg.get("LOSS_LOC_BETA")
    if kind is None:
        if beta is not None:
            raise ValueError("LOSS_LOC_BETA is given without LOSS_LOC_TYPE")
        return None
    if not (isinstance(kind, str) and kind in LOC_LOSS_TYPES):
        raise ValueError("LOSS_LOC_TYPE must be one of %s, got %r" % (", ".join(LOC_LOSS_TYPES), kind))
    if kind != "smooth_l1":
        if beta is not None:
            raise ValueError("LOSS_LOC_BETA goes with LOSS_LOC_TYPE smooth_l1 only, got it with %s" % kind)
        return kind, None
    if beta is None:
        return kind, 0.1
    if not (isinstance(beta, (int, float)) and not isinstance(beta, bool) and 0 < ctypes.c_float(beta).value < float("inf")):
        raise ValueError("LOSS_LOC_BETA must be a finite number > 0, got %r" % (beta,))
    return kind, float(beta)


QUALITY_TARGETS = ("qfl", "varifocal")                       # MBX_QUALITY_QFL = 1, MBX_QUALITY_VFL = 2 (include/mbx.h)


def quality_loss(cfg):
    """An IoU-aware confidence target (mbx_loss_fwd_bwd_quality; not in the reference, so off when absent): None, or a dict
    of Trainer keyword arguments.
      LOSS_QUALITY_TARGET      qfl (the Quality Focal Loss of Generalized Focal Loss, Li et al. 2020) or varifocal (the
        Varifocal Loss of VarifocalNet, Zhang et al. 2021); absent or null = off.  A positive trains its confidence towards
        the IoU of its prediction with its box; the scores then estimate localisation quality as well as objectness.
      LOSS_QUALITY_GAMMA       a number in [0, 10], under qfl 0 or >= 1 (|q - s|^(gamma-1) is unbounded below 1); default 2.0;
        only with the target.
      LOSS_QUALITY_NEG_WEIGHT  finite and > 0 as a float32; default 1.0 under qfl and 0.75 under varifocal, the papers'
        settings; only with the target.
    LOSS_FOCAL_GAMMA or LOSS_FOCAL_ALPHA beside the target raises ValueError naming both keys: each decides the confidence
    term.  A bool, a string where a number is expected, a list, a NaN, a value out of range or a dependent key without the
    target raises ValueError naming the key.  Composes with LOSS_LOC_TYPE, LOSS_NEG_PER_POS and the matching keys.  Host code
    only."""
    number = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool)
    target, gamma, w_neg = cfg.get("LOSS_QUALITY_TARGET"), cfg.get("LOSS_QUALITY_GAMMA"), cfg.get("LOSS_QUALITY_NEG_WEIGHT")
    if target is None:
        for key, v in (("LOSS_QUALITY_GAMMA", gamma), ("LOSS_QUALITY_NEG_WEIGHT", w_neg)):
            if v is not None:
                raise ValueError("%s is given without LOSS_QUALITY_TARGET" % key)
        return None
    if not (isinstance(target, str) and target in QUALITY_TARGETS):
        raise ValueError("LOSS_QUALITY_TARGET must be one of %s, got %r" % (", ".join(QUALITY_TARGETS), target))
    for key in ("LOSS_FOCAL_GAMMA", "LOSS_FOCAL_ALPHA"):
        if cfg.get(key) is not None:
            raise ValueError("LOSS_QUALITY_TARGET and %s are both given: each decides the confidence term" % key)
    if gamma is None:
        gamma = 2.0
    elif not (number(gamma) and 0 <= gamma <= 10):
        raise ValueError("LOSS_QUALITY_GAMMA must be a number in [0, 10], got %r" % (gamma,))
    elif target == "qfl" and 0 < gamma < 1:
        raise ValueError("LOSS_QUALITY_GAMMA must be 0 or >= 1 under LOSS_QUALITY_TARGET qfl, got %r" % (gamma,))
    if w_neg is None:
        w_neg = 1.0 if target == "qfl" else 0.75
    elif not (number(w_neg) and 0 < ctypes.c_float(w_neg).value < float("inf")):
        raise ValueError("LOSS_QUALITY_NEG_WEIGHT must be a finite number > 0 as a float32, got %r" % (w_neg,))
    return {"quality_target": target, "quality_gamma": float(gamma), "quality_neg_weight": float(w_neg)}


IGNORE_SOURCES = ("prior", "prediction")


def ignore_band(cfg):
    """An ignore band for near-object priors in the confidence loss (mbx_match_ignore / mbx_loss_fwd_bwd_ignore; not in the
    reference, so off when absent): None, or a dict of Trainer keyword arguments.
      LOSS_IGNORE_IOU_THRESHOLD  a number in (0, 1]; absent or null = off.  A prior the matching left free that overlaps some
        box of its image by at least the key adds nothing to the confidence loss, gets no gradient and is neither a
        candidate nor a positive for mining (RetinaNet's band: positive at or over 0.5, negative under 0.4, neither between).
      LOSS_IGNORE_SOURCE         prior (default): the overlap is the prior's own; prediction: the decoded prediction's
        (YOLOv3's rule).  Only with the threshold.
    Together with LOSS_MATCH_IOU_THRESHOLD and source prior, a threshold above the matching threshold raises ValueError
    naming both keys: every free prior is at or under the matching threshold, so the band would be empty.  A bool, a
    string, a list, a NaN or a value outside (0, 1] for the threshold, a source that is no such string, or the source
    without the threshold raises ValueError naming the key.  Composes with LOSS_MATCH_ATSS_TOPK, LOSS_NEG_PER_POS, the focal,
    location and quality keys.  Host code only."""
    v, source = cfg.get("LOSS_IGNORE_IOU_THRESHOLD"), cfg.get("LOSS_IGNORE_SOURCE")
    if v is None:
        if source is not None:
            raise ValueError("LOSS_IGNORE_SOURCE is given without LOSS_IGNORE_IOU_THRESHOLD")
        return None
    if not (isinstance(v, (int, float)) and not isinstance(v, bool) and 0 < v <= 1):
        raise ValueError("LOSS_IGNORE_IOU_THRESHOLD must be a number in (0, 1], got %r" % (v,))
    if source is None:
        source = "prior"
    elif not (isinstance(source, str) and source in IGNORE_SOURCES):
        raise ValueError("LOSS_IGNORE_SOURCE must be one of %s, got %r" % (", ".join(IGNORE_SOURCES), source))
    hi = match_iou_threshold(cfg)
    if hi is not None and source == "prior" and v > hi:
        raise ValueError("LOSS_IGNORE_IOU_THRESHOLD %r is above LOSS_MATCH_IOU_THRESHOLD %r: no free prior overlaps a box by "
                         "that much, the band would be empty" % (v, hi))
    return {"ignore_iou_threshold": float(v), "ignore_source": source}


def grad_clip(cfg):
    """Global-norm gradient clipping and the non-finite-step guard (mbx_grad_sqnorm / mbx_clip_finalize /
    mbx_rmsprop_ema_step_clipped; not in the reference, so off when absent): None, or CLIP_GRADIENT_NORM as a float > 0
    (absent or null = off; .inf = never clip, only skip steps whose gradient is not finite).  The clipped vector is the one
    the optimiser consumes, g + WEIGHT_DECAY * w over the trainable filters and g over the trainable betas: what
    tf.clip_by_global_norm would see on the reference's total_loss, which contains slim's regulariser.  A bool, a string, a
    list, a NaN or a value <= 0 raises ValueError naming the key.  Host code only."""
    v = cfg.get("CLIP_GRADIENT_NORM")
    if v is None:
        return None
    if not (isinstance(v, (int, float)) and not isinstance(v, bool) and v > 0):
        raise ValueError("CLIP_GRADIENT_NORM must be a number > 0 (.inf = guard only), got %r" % (v,))
    return float(v)


OPTIMIZERS = ("rmsprop", "sgd", "adam", "adamw")
_ADAM_KEYS = ("ADAM_BETA1", "ADAM_BETA2", "ADAM_EPSILON")
# the keys each rule reads (the RMSPROP_* keys sit in DEFAULTS and are ignored under the other rules)
OPTIMIZER_KEYS = {"rmsprop": (), "sgd": ("SGD_MOMENTUM", "SGD_NESTEROV"), "adam": _ADAM_KEYS, "adamw": _ADAM_KEYS + ("ADAMW_WEIGHT_DECAY",)}


def check_optimizer_args(optimizer, sgd_momentum=0.9, adam_beta1=0.9, adam_beta2=0.999, adam_epsilon=1e-8, adamw_weight_decay=0.01):
    """The ranges optimizer() holds the config keys to, on the Trainer's keyword arguments (whichever rule is chosen):
    raises ValueError naming the argument."""
    number = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool)
    if optimizer not in OPTIMIZERS:
        raise ValueError("optimizer must be one of %s, got %r" % (", ".join(OPTIMIZERS), optimizer))
    for what, v in (("sgd_momentum", sgd_momentum), ("adam_beta1", adam_beta1), ("adam_beta2", adam_beta2)):
        if not (number(v) and 0 <= v < 1):
            raise ValueError("%s must be a number in [0, 1), got %r" % (what, v))
    if not (number(adam_epsilon) and 0 < ctypes.c_float(adam_epsilon).value < float("inf")):
        raise ValueError("adam_epsilon must be a finite number > 0 as a float32, got %r" % (adam_epsilon,))
    if not (number(adamw_weight_decay) and 0 <= ctypes.c_float(adamw_weight_decay).value < float("inf")):
        raise ValueError("adamw_weight_decay must be a finite number >= 0, got %r" % (adamw_weight_decay,))


def optimizer(cfg):
    """The update rule (mbx_sgd_ema_step / mbx_adam_ema_step; the reference has RMSProp alone, so off when absent) and the
    learning-rate warm-up: a dict of Trainer keyword arguments, empty when neither key is set.
      OPTIMIZER  absent, null or rmsprop: the reference's step under the RMSPROP_* keys.
        sgd    tf.train.MomentumOptimizer on total_loss: SGD_MOMENTUM (a number in [0, 1), default 0.9), SGD_NESTEROV (a bool,
               default false).
        adam   Adam on total_loss, the L2 term in the gradient: ADAM_BETA1 (in [0, 1), default 0.9), ADAM_BETA2 (in [0, 1),
               default 0.999), ADAM_EPSILON (finite and > 0 as a float32, default 1e-8).
        adamw  the adam keys and ADAMW_WEIGHT_DECAY (finite and >= 0, default 0.01): decoupled decay of the trainable filters;
               the coupled L2 term leaves the loss and the gradient.
      LEARNING_RATE_WARMUP_STEPS  an int >= 0 (absent, null or 0 = off), with any rule: the learning rate of step t is the
        schedule's times min(1, (t + 1) / warmup).
    A key of another rule than the chosen one, a bool where a number is expected (or the reverse), a string, a list, a NaN
    or a value out of range raises ValueError naming the key.  Host code only."""
    number = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool)
    kind = cfg.get("OPTIMIZER")
    if kind is not None and not (isinstance(kind, str) and kind in OPTIMIZERS):
        raise ValueError("OPTIMIZER must be one of %s, got %r" % (", ".join(OPTIMIZERS), kind))
    own = OPTIMIZER_KEYS[kind or "rmsprop"]
    for keys in OPTIMIZER_KEYS.values():
        for key in keys:
            if key not in own and cfg.get(key) is not None:
                raise ValueError("%s does not go with OPTIMIZER %s" % (key, kind or "rmsprop (the default)"))
    out = {}
    if kind is not None:
        out["optimizer"] = kind

    def unit(key, default):                                   # a number in [0, 1)
        v = cfg.get(key)
        if v is None:
            return default
        if not (number(v) and 0 <= v < 1):
            raise ValueError("%s must be a number in [0, 1), got %r" % (key, v))
        return float(v)
    if kind == "sgd":
        nesterov = cfg.get("SGD_NESTEROV")
        if nesterov is not None and not isinstance(nesterov, bool):
            raise ValueError("SGD_NESTEROV must be true or false, got %r" % (nesterov,))
        out.update(sgd_momentum=unit("SGD_MOMENTUM", 0.9), sgd_nesterov=bool(nesterov))
    elif kind in ("adam", "adamw"):
        eps = cfg.get("ADAM_EPSILON")
        if eps is not None and not (number(eps) and 0 < ctypes.c_float(eps).value < float("inf")):
            raise ValueError("ADAM_EPSILON must be a finite number > 0 as a float32, got %r" % (eps,))
        out.update(adam_beta1=unit("ADAM_BETA1", 0.9), adam_beta2=unit("ADAM_BETA2", 0.999),
                   adam_epsilon=1e-8 if eps is None else float(eps))
        if kind == "adamw":
            wd = cfg.get("ADAMW_WEIGHT_DECAY")
            if wd is not None and not (number(wd) and 0 <= ctypes.c_float(wd).value < float("inf")):
                raise ValueError("ADAMW_WEIGHT_DECAY must be a finite number >= 0, got %r" % (wd,))
            out["adamw_weight_decay"] = 0.01 if wd is None else float(wd)
    if cfg.get("LEARNING_RATE_WARMUP_STEPS") is not None:
        warmup = _int_key(cfg, "LEARNING_RATE_WARMUP_STEPS", 0)
        if warmup:
            out["lr_warmup_steps"] = warmup
    return out


def trust_coeff_default(optimizer):
    """LAYERWISE_TRUST_COEFF when absent: LARS's eta under sgd, 1 under adam / adamw (LAMB has no such factor)."""
    return 0.001 if optimizer == "sgd" else 1.0


def check_trust_args(optimizer, layerwise_trust=False, trust_coeff=None):
    """The ranges layerwise_trust() holds the config keys to, on the Trainer's keyword arguments: raises ValueError naming
    the argument.  Returns the coefficient in use, or None when the switch is off."""
    if not isinstance(layerwise_trust, bool):
        raise ValueError("layerwise_trust must be True or False, got %r" % (layerwise_trust,))
    if not layerwise_trust:
        if trust_coeff is not None:
            raise ValueError("trust_coeff goes with layerwise_trust=True only, got %r" % (trust_coeff,))
        return None
    if optimizer not in ("sgd", "adam", "adamw"):
        raise ValueError("layerwise_trust goes with optimizer sgd (LARS), adam or adamw (LAMB), not with %r" % (optimizer,))
    if trust_coeff is None:
        return trust_coeff_default(optimizer)
    if not (isinstance(trust_coeff, (int, float)) and not isinstance(trust_coeff, bool) and 0 < ctypes.c_float(trust_coeff).value < float("inf")):
        raise ValueError("trust_coeff must be a finite number > 0 as a float32, got %r" % (trust_coeff,))
    return float(trust_coeff)


def layerwise_trust(cfg):
    """Layer-wise trust ratios (mbx_trust_* / mbx_sgd_ema_step_trust / mbx_adam_ema_step_trust; not in the reference, so off
    when absent): None, or a dict of Trainer keyword arguments.
      LAYERWISE_TRUST        a bool (absent, null or false = off).  Every trainable filter variable with more than one
        dimension scales its update by LAYERWISE_TRUST_COEFF * ||w|| / ||x||: with OPTIMIZER sgd this is LARS (x = g', the
        vector the optimiser consumes), with adam / adamw LAMB (x = Adam's update, the decoupled decay included).  Biases and
        betas keep a ratio of 1.  With OPTIMIZER absent or rmsprop: ValueError.
      LAYERWISE_TRUST_COEFF  finite and > 0 as a float32, only with LAYERWISE_TRUST: true; default 0.001 under sgd (LARS's
        eta), 1.0 under adam / adamw.
    A non-bool switch, a bool, a string, a list, a NaN or a value out of range for the coefficient, or the coefficient
    without the switch raises ValueError naming the key.  Host code only."""
    on, coeff = cfg.get("LAYERWISE_TRUST"), cfg.get("LAYERWISE_TRUST_COEFF")
    if on is not None and not isinstance(on, bool):
        raise ValueError("LAYERWISE_TRUST must be true or false, got %r" % (on,))
    if not on:
        if coeff is not None:
            raise ValueError("LAYERWISE_TRUST_COEFF goes with LAYERWISE_TRUST: true only, got %r" % (coeff,))
        return None
    kind = cfg.get("OPTIMIZER")
    if kind not in ("sgd", "adam", "adamw"):
        raise ValueError("LAYERWISE_TRUST goes with OPTIMIZER sgd (LARS), adam or adamw (LAMB), not with OPTIMIZER %s"
                         % (kind if kind is not None else "absent (rmsprop)",))
    if coeff is None:
        return {"layerwise_trust": True, "trust_coeff": trust_coeff_default(kind)}
    if not (isinstance(coeff, (int, float)) and not isinstance(coeff, bool) and 0 < ctypes.c_float(coeff).value < float("inf")):
        raise ValueError("LAYERWISE_TRUST_COEFF must be a finite number > 0 as a float32, got %r" % (coeff,))
    return {"layerwise_trust": True, "trust_coeff": float(coeff)}

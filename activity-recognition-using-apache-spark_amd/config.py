"""Run configuration: dataclass + CLI + presets.

The reference has no config system — every hyper-parameter is a literal in
``Main/main.py`` (split ``:80``, LR ``:115``, CV grid ``:202-204``, DT ``:297``, RF ``:478``)
and the Spark master is an undefined variable (``:8``).  ``RunConfig`` defaults
reproduce those literals exactly (preset ``reference``); other presets cover the
BASELINE.json configurations.  Presets can also be loaded from YAML
(``--preset-file``, parsed with ``yaml.safe_load``).
"""
from __future__ import annotations

import argparse
import dataclasses
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import os as _os

_REF_WISDM = "/root/reference/Main/wisdm_main_ver_0.0/data/wisdm_data.csv"
_VENDORED_WISDM = _os.path.join(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))), "tests", "data",
                                "wisdm_data.csv")
DEFAULT_WISDM = _REF_WISDM if _os.path.exists(_REF_WISDM) else _VENDORED_WISDM


@dataclass
class RunConfig:
    data: str = DEFAULT_WISDM
    out_dir: str = "wisdm_main_ver_0.0/main_result"
    plot_dir: str = "wisdm_main_ver_0.0/plot"
    encoding: str = "reference"            # reference | numeric43 | rocket | numeric43+rocket | raw
    classifiers: List[str] = field(default_factory=lambda: ["lr", "lrcv", "dt", "dtcv", "rf", "rfcv"])
    split: List[float] = field(default_factory=lambda: [0.7, 0.3])
    seed: int = 2018
    device: str = "auto"
    # on a GPU: parse + dictionary-encode the CSV with the HIP kernels and keep the table in HBM
    # (the feature pipeline then runs on the device); --no-csv-device keeps the host parser
    csv_device: bool = True
    # raw accelerometer rows (user,activity,timestamp,x,y,z) instead of the pre-windowed table:
    # windowed + featurized on the device into the WISDM columns (features/raw.py)
    raw: Optional[str] = None
    hz: float = 20.0                       # WISDM v1.1 sampling rate (BASELINE.json configs use 50)
    window_sec: float = 10.0               # WISDM window length
    overlap: float = 0.0                   # fraction of a window shared with the next one
    # RocketFeaturizer (new, opt-in, needs --raw): --rocket N appends ~N MiniRocket-style RKT* columns
    rocket: int = 0
    # StreamFilter (new, opt-in, needs --raw): Butterworth conditioning of the samples before they are windowed
    filter: str = ""                       # lowpass | gravity | body
    filter_cutoff: float = 0.0             # Hz; 0 = the kind's default (hz / 4 for lowpass, 0.3 for gravity / body)
    filter_order: int = 3
    filter_zero_phase: bool = False        # forwards and backwards over every (user, activity) run
    # LogisticRegression (main.py:115)
    lr_max_iter: int = 20
    lr_reg: float = 0.3
    lr_elastic_net: float = 0.0
    # armijo (default) | wolfe: the uncentred RKT* columns (mean / std up to ~30) need the Wolfe search, the
    # batched Armijo trials reject every step from the start there
    lr_line_search: str = "armijo"
    # CrossValidator (main.py:202-212)
    cv_folds: int = 5
    cv_reg_grid: List[float] = field(default_factory=lambda: [0.1, 0.3, 0.5])
    cv_en_grid: List[float] = field(default_factory=lambda: [0.0, 0.1, 0.2])
    cv_metric: str = "accuracy"            # reference behaviour: "mae" (RegressionEvaluator leak, main.py:175)
    # DecisionTree (main.py:297) / RandomForest (main.py:478)
    dt_max_depth: int = 3
    rf_num_trees: int = 100
    rf_max_depth: int = 4
    max_bins: int = 32
    # RF over N ranks (torchrun): "tree" = every rank all rows, numTrees / N trees, one all-gather;
    # "data" = row shards + per-level owner reduction; "auto" = tree while the table is small
    rf_parallel: str = "auto"
    # GBTClassifier (new): multinomial Newton boosting, K trees per round
    gbt_max_iter: int = 20
    gbt_max_depth: int = 5
    gbt_step_size: float = 0.1
    # KNNClassifier (new): exact k-nearest neighbours; --knn-group-col UID adds the leave-one-group-out
    # accuracy over the training table (one grouped search)
    knn_k: int = 5
    knn_weights: str = "uniform"             # uniform | distance
    knn_group_col: str = ""
    # DTWClassifier (new, needs --raw and --encoding raw): nearest neighbours between raw windows under banded
    # dynamic time warping; --dtw-group-col USER adds the leave-one-group-out accuracy over the training table
    dtw_k: int = 1
    dtw_band: float = 0.1                    # Sakoe-Chiba radius as a fraction of the window
    dtw_weights: str = "uniform"             # uniform | distance
    dtw_normalize: str = "none"              # none | zscore (per window and axis)
    dtw_group_col: str = ""
    # RidgeClassifier (new): Gram-moment ridge, the penalty chosen by one-pass k-fold cross-validation
    ridge_alphas: List[float] = field(default_factory=lambda: [round(10.0 ** (-3 + 6 * i / 9), 12) for i in range(10)])
    ridge_folds: int = 5
    # NaiveBayes / MLP (new)
    nb_model_type: str = "gaussian"
    mlp_hidden: List[int] = field(default_factory=lambda: [128, 128])
    mlp_epochs: int = 60
    mlp_batch: int = 256
    mlp_lr: float = 2e-3
    # HMMSmoother (new, opt-in): Viterbi-smoothed timeline of every classifier's test predictions
    hmm: bool = False
    hmm_sequence_col: str = "USER"
    hmm_emission: str = "scaled"             # scaled (p / prior) | posterior
    hmm_posterior: bool = False              # + forward-backward posteriors of the test predictions (implies hmm)
    hmm_em_iter: int = 0                     # Baum-Welch iterations on the first classifier's training predictions
    # KMeans + silhouette ClusteringEvaluator (new, opt-in): --kmeans K clusters the training rows' dense
    # numeric features after the classifiers
    kmeans: int = 0
    kmeans_max_iter: int = 20
    kmeans_init: str = "k-means++"           # k-means++ | random
    # GaussianMixture (new, opt-in): --gmm K fits a K-component mixture on the same dense numeric features
    gmm: int = 0
    gmm_max_iter: int = 100
    gmm_cov: str = "full"                    # full | diag
    gmm_init: str = "k-means"                # k-means | random
    # artefacts
    plots: bool = False
    report: bool = False                   # Results table + charts + index.html (report/summary.py)
    save_models: Optional[str] = None
    append_csv: bool = False
    echo: bool = False


PRESETS: Dict[str, Dict] = {
    "reference": {},
    # BASELINE.json config 1: LR on CPU (plumbing)
    "lr-cpu": {"classifiers": ["lr"], "device": "cpu"},
    # BASELINE.json config 2: RF 100 trees depth 10 on one GPU
    "rf-deep": {"classifiers": ["rf"], "rf_max_depth": 10, "encoding": "numeric43"},
    # BASELINE.json config 3: 3-layer MLP (bf16 on GPU)
    "mlp": {"classifiers": ["mlp"], "encoding": "numeric43"},
    # everything the framework offers on the better encoding
    "all-numeric": {"classifiers": ["lr", "dt", "rf", "nb", "mlp"], "encoding": "numeric43", "rf_max_depth": 10},
    # gradient-boosted trees on the numeric encoding
    "gbt": {"classifiers": ["gbt"], "encoding": "numeric43"},
    # exact k-nearest neighbours on the numeric encoding
    "knn": {"classifiers": ["knn"], "encoding": "numeric43"},
    # convolutional window features of a raw stream (--raw PATH) under logistic regression
    "rocket": {"classifiers": ["lr"], "encoding": "rocket", "rocket": 1680, "lr_max_iter": 100, "lr_reg": 0.01,
               "lr_line_search": "wolfe"},
    # the same columns under the ridge classifier of the Rocket literature (cross-validated penalty)
    "rocket-ridge": {"classifiers": ["ridge"], "encoding": "rocket", "rocket": 1680},
    # nearest neighbours between the raw windows of a stream (--raw PATH) under banded dynamic time warping
    "dtw": {"classifiers": ["dtw"], "encoding": "raw"},
}


def _list(t):
    return lambda s: [t(x) for x in s.split(",") if x != ""]


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="MI355X-native WISDM activity recognition (reference: Main/main.py)")
    ap.add_argument("--preset", default="reference", choices=sorted(PRESETS))
    ap.add_argument("--preset-file", default=None, help="YAML file with RunConfig fields")
    d = RunConfig()
    for f in dataclasses.fields(RunConfig):
        name = "--" + f.name.replace("_", "-")
        default = getattr(d, f.name)
        if isinstance(default, bool):
            ap.add_argument(name, dest=f.name, action=argparse.BooleanOptionalAction, default=None)
        elif isinstance(default, list):
            t = float if (default and isinstance(default[0], float)) else (int if default and isinstance(default[0], int) else str)
            ap.add_argument(name, dest=f.name, type=_list(t), default=None)
        elif f.name == "hmm_em_iter":  # spelled out: "--hmm-em" alone would also abbreviate --hmm-emission
            ap.add_argument("--hmm-em", name, dest=f.name, type=int, default=None)
        else:
            ap.add_argument(name, dest=f.name, type=type(default) if default is not None else str, default=None)
    return ap


def config_from_args(argv=None) -> RunConfig:
    ap = build_parser()
    a = ap.parse_args(argv)
    cfg = RunConfig()
    for k, v in PRESETS[a.preset].items():
        setattr(cfg, k, v)
    if a.preset_file:
        import yaml

        with open(a.preset_file) as fh:
            for k, v in (yaml.safe_load(fh) or {}).items():
                if not hasattr(cfg, k):
                    raise KeyError(f"unknown config key {k}")
                setattr(cfg, k, v)
    for f in dataclasses.fields(RunConfig):
        v = getattr(a, f.name)
        if v is not None:
            setattr(cfg, f.name, v)
    if cfg.rocket < 0 or (cfg.rocket > 0 and not cfg.raw):
        ap.error("--rocket N (and the rocket preset) featurize a raw stream: give --raw PATH and N > 0")
    filter_given = cfg.filter or cfg.filter_cutoff != 0.0 or cfg.filter_order != 3 or cfg.filter_zero_phase
    if filter_given and not cfg.raw:
        ap.error("--filter (and --filter-cutoff / --filter-order / --filter-zero-phase) condition a raw stream: give --raw PATH")
    if filter_given and cfg.filter not in ("lowpass", "gravity", "body"):
        ap.error(f"--filter takes lowpass, gravity or body, got {cfg.filter!r}")
    if cfg.filter and (not 1 <= cfg.filter_order <= 4 or cfg.filter_cutoff < 0.0 or cfg.filter_cutoff >= cfg.hz / 2):
        ap.error("--filter-order takes 1..4 and --filter-cutoff a frequency below hz / 2")
    if "rocket" in cfg.encoding and cfg.rocket == 0:
        ap.error(f"--encoding {cfg.encoding} needs --rocket N")
    if (cfg.encoding == "raw" or "dtw" in cfg.classifiers) and not cfg.raw:
        ap.error("--encoding raw (and the dtw preset) compare the windows of a raw stream: give --raw PATH")
    if "dtw" in cfg.classifiers and cfg.encoding != "raw":
        ap.error("the dtw classifier takes --encoding raw")
    if cfg.hmm_posterior or cfg.hmm_em_iter > 0:  # both are switches OF the smoother
        cfg.hmm = True
    return cfg

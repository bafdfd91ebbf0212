#!/usr/bin/env python3
"""``main.py`` — the reference entry point (``Main/main.py``), MI355X-native.

Same flow and artefacts as the PySpark script: load the WISDM CSV, print the
schema / sample / class counts / describe, run the feature pipeline, split
70/30 (seed 2018), train and evaluate LogisticRegression, LR+CrossValidator,
DecisionTree(+CV), RandomForest(+CV) — plus NaiveBayes and an MLP — and write
``result.txt``, ``additional_param.csv``, ``crossFold_additional_param.csv``
(identical headers), a ``metrics.jsonl`` record and optional plots / saved models.

    python main.py                                  # the reference run (all six models)
    python main.py --classifiers lr --device cpu     # BASELINE config 1 (plumbing)
    python main.py --preset rf-deep                  # RF 100 trees x depth 10 on the GPU
    python main.py --preset all-numeric --save-models models/
    python main.py --preset gbt --gbt-max-iter 50    # gradient-boosted trees (K trees per round)
    python main.py --preset knn --knn-k 5 --knn-group-col UID   # exact k-nearest neighbours + leave-one-group-out
    python main.py --hmm --save-models models/       # + Viterbi-smoothed timeline per classifier (HMMSmoother)
    python main.py --hmm-posterior --hmm-em 10       # + forward-backward posteriors; Baum-Welch-refined transitions
    python main.py --kmeans 6 --save-models models/  # + KMeans clusters, silhouette, purity against the labels
    python main.py --csv-device                      # CSV parsed + dictionary-encoded by the HIP kernels
    python main.py --report                          # + Results table, charts and index.html (report/)
    python main.py --raw raw.csv --hz 20 --window-sec 10 --overlap 0.5   # raw user,activity,timestamp,x,y,z rows
    python main.py --raw raw.csv --preset rocket --save-models models/    # + MiniRocket-style RKT* columns under LR (models/rocket)
    python main.py --raw raw.csv --preset rocket-ridge --ridge-folds 5    # the same columns under RidgeClassifier (CV-chosen penalty)
    python main.py --raw raw.csv --preset dtw --dtw-group-col USER        # nearest neighbours between raw windows under banded DTW
    python main.py --raw raw.csv --filter body --filter-cutoff 0.3 --save-models models/   # Butterworth-conditioned samples (models/filter)
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 main.py   # data parallel over 8 GPUs (RCCL)

Under ``torch.distributed.run`` every rank loads the (small) table and every model is
fit data-parallel on the rank's row shard (``har.models.base.data_parallel``): one
all-reduce per L-BFGS evaluation for LR / LR-CV, owner-computed tree levels
(reduce-scatter + all-gather) for DT / RF (+CV), gradient all-reduce for the MLP,
one moment all-reduce for NaiveBayes.  Rank 0 writes the artefacts.

Paths default to the reference layout relative to the working directory
(``wisdm_main_ver_0.0/main_result``); ``--data`` points at the CSV.
"""
from __future__ import annotations

import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from har.config import RunConfig, config_from_args  # noqa: E402
from har.data.csv_io import read_csv  # noqa: E402
from har.data.split import random_split  # noqa: E402
from har.data.table import describe_text  # noqa: E402
from har.evaluation.evaluators import evaluate_all  # noqa: E402
from har.features import wisdm  # noqa: E402
from har.models.base import data_parallel, features_tensor, resolve_device  # noqa: E402
from har.parallel import dist as hdist  # noqa: E402
from har.report import csvout  # noqa: E402
from har.report.text import (BANNER_CLASSIFY, BANNER_PIPELINE, BANNER_TRAIN, RunLog, evaluation_block,  # noqa: E402
                             model_header, section)
from har.suite import build_estimator, n_feature_columns, warm_up_device  # noqa: E402
from har.utils import persist  # noqa: E402
from har.utils.timing import PhaseTimer, device_sync  # noqa: E402


def make_estimator(name: str, cfg: RunConfig, dev, n_features: int, n_classes: int):
    """``build_estimator`` plus the classifiers added after the reference suite (``gbt``, ``knn``, ``ridge``, ``dtw``)."""
    if name == "ridge":
        from har.models.ridge import RidgeClassifier

        return RidgeClassifier(alphas=cfg.ridge_alphas, numFolds=cfg.ridge_folds, seed=cfg.seed, featuresCol="features",
                               labelCol="label", device=dev)
    if name == "knn":
        from har.models.knn import KNNClassifier

        return KNNClassifier(k=cfg.knn_k, weights=cfg.knn_weights, featuresCol="features", labelCol="label", device=dev)
    if name == "dtw":
        from har.models.dtw import DTWClassifier

        return DTWClassifier(k=cfg.dtw_k, band=cfg.dtw_band, weights=cfg.dtw_weights, normalize=cfg.dtw_normalize,
                             axes=3, featuresCol="features", labelCol="label", device=dev)
    if name == "gbt":
        from har.models.gbt import GBTClassifier

        return GBTClassifier(featuresCol="features", labelCol="label", maxIter=cfg.gbt_max_iter,
                             maxDepth=cfg.gbt_max_depth, stepSize=cfg.gbt_step_size, maxBins=cfg.max_bins,
                             seed=cfg.seed, device=dev)
    return build_estimator(name, cfg, dev, n_features, n_classes)


def run_kmeans(cfg: RunConfig, dev, ctx, train, test, vocab, timer, log, main_rank) -> dict:
    """``--kmeans K``: cluster the training rows' dense numeric features, then the block of result.txt —
    sizes, cost, iterations, silhouette on the test rows, purity and the cluster-by-label table."""
    from har.evaluation.evaluators import ClusteringEvaluator
    from har.models.kmeans import KMeans, kmeans_feature_cols, table_features

    cols = kmeans_feature_cols(cfg.encoding)
    X_train, X_test = table_features(train, cols, dev), table_features(test, cols, dev)
    y_train = torch.as_tensor(train["label"].data.astype(np.int64), device=dev)
    est = KMeans(k=cfg.kmeans, maxIter=cfg.kmeans_max_iter, initMode=cfg.kmeans_init, seed=cfg.seed, device=dev)
    with timer.phase("fit:kmeans"), data_parallel(ctx):
        model = est.fit_features(X_train)
    model.feature_cols = cols
    train_s = round(timer.get("fit:kmeans"), 6)
    with timer.phase("evaluate:kmeans"):
        cm, majority, purity = model.label_map(model.predict(X_train), y_train, len(vocab))
        pred_test = model.predict(X_test)
        sil = ClusteringEvaluator(device=dev).evaluate_tensors(X_test, pred_test, model.k) if X_test.shape[0] else 0.0
    s = model.summary
    section(log, "KMeans")
    log.print(f"{model} trained in {train_s} seconds ({X_train.shape[1]} features, init {cfg.kmeans_init})")
    log.print("Cluster Sizes      = " + str(s.clusterSizes))
    log.print("Training Cost      = %g" % s.trainingCost)
    log.print("Iterations         = %d (converged: %s)" % (s.numIter, s.converged))
    log.print("Silhouette (test)  = %g" % sil)
    log.print("Purity (train)     = %g" % purity)
    log.print("Cluster x label (rows: clusters; columns: " + ", ".join(str(v) for v in vocab) + ")")
    for c, row in enumerate(cm.tolist()):
        log.print("  %3d -> %-12s %s" % (c, vocab[int(majority[c])], row))
    if cfg.save_models and main_rank:
        persist.save(model, os.path.join(cfg.save_models, "kmeans"), labels=vocab)
    return {"model": str(model), "k": model.k, "train_s": train_s, "training_cost": s.trainingCost,
            "num_iter": s.numIter, "converged": s.converged, "cluster_sizes": s.clusterSizes, "silhouette": sil,
            "purity": purity, "contingency": cm.tolist(), "majority_labels": model.majority_labels}


def run_gmm(cfg: RunConfig, dev, train, test, vocab, timer, log, main_rank) -> dict:
    """``--gmm K``: a K-component Gaussian mixture on the training rows' dense numeric features (every rank
    fits the whole table), then the block of result.txt — weights, sizes, log-likelihood, iterations, the
    mean test log-likelihood, silhouette on the test rows, purity and the cluster-by-label table."""
    from har.evaluation.evaluators import ClusteringEvaluator
    from har.models.gmm import GaussianMixture
    from har.models.kmeans import kmeans_feature_cols, table_features

    cols = kmeans_feature_cols(cfg.encoding)
    X_train, X_test = table_features(train, cols, dev), table_features(test, cols, dev)
    y_train = torch.as_tensor(train["label"].data.astype(np.int64), device=dev)
    est = GaussianMixture(k=cfg.gmm, maxIter=cfg.gmm_max_iter, covarianceType=cfg.gmm_cov, initMode=cfg.gmm_init,
                          seed=cfg.seed, device=dev)
    with timer.phase("fit:gmm"):
        model = est.fit_tensors(X_train)
    model.feature_cols = cols
    train_s = round(timer.get("fit:gmm"), 6)
    with timer.phase("evaluate:gmm"):
        cm, majority, purity = model.label_map(model.summary.predictions.long(), y_train, len(vocab))
        n_test = X_test.shape[0]
        pred_test = model.predict(X_test)
        test_ll = float(model.score_samples(X_test).mean()) if n_test else 0.0
        sil = ClusteringEvaluator(device=dev).evaluate_tensors(X_test, pred_test, model.k) if n_test else 0.0
    s = model.summary
    section(log, "GaussianMixture")
    log.print(f"{model} trained in {train_s} seconds ({X_train.shape[1]} features, {cfg.gmm_cov} covariances, "
              f"init {cfg.gmm_init})")
    log.print("Weights            = " + str([round(float(v), 6) for v in model.weights.tolist()]))
    log.print("Cluster Sizes      = " + str(s.clusterSizes))
    log.print("Log-Likelihood     = %g" % s.logLikelihood)
    log.print("Iterations         = %d (converged: %s)" % (s.numIter, s.converged))
    log.print("Mean LL / row (test) = %g" % test_ll)
    log.print("Silhouette (test)  = %g" % sil)
    log.print("Purity (train)     = %g" % purity)
    log.print("Cluster x label (rows: clusters; columns: " + ", ".join(str(v) for v in vocab) + ")")
    for c, row in enumerate(cm.tolist()):
        log.print("  %3d -> %-12s %s" % (c, vocab[int(majority[c])], row))
    if cfg.save_models and main_rank:
        persist.save(model, os.path.join(cfg.save_models, "gmm"), labels=vocab)
    return {"model": str(model), "k": model.k, "train_s": train_s, "log_likelihood": s.logLikelihood,
            "num_iter": s.numIter, "converged": s.converged, "cluster_sizes": s.clusterSizes,
            "weights": model.weights.tolist(), "test_mean_log_likelihood": test_ll, "silhouette": sil, "purity": purity,
            "contingency": cm.tolist(), "majority_labels": model.majority_labels}


def run(cfg: RunConfig, ctx=None) -> dict:
    dev = ctx.device if ctx is not None else resolve_device(None if cfg.device == "auto" else cfg.device)
    main_rank = ctx is None or ctx.is_main
    os.makedirs(cfg.out_dir, exist_ok=True)
    log = RunLog(os.path.join(cfg.out_dir, "result.txt") if main_rank else os.devnull, echo=cfg.echo and main_rank)
    t_run = time.perf_counter()
    timer = PhaseTimer(dev)

    log.print("Loading Data Set...")
    stream_filter = None
    with timer.phase("load_csv"):
        if cfg.raw:  # raw sensor rows -> device windowing + featurization -> the WISDM table
            from har.features.raw import raw_to_table

            if cfg.filter:
                from har.features.filter import StreamFilter

                stream_filter = StreamFilter(cfg.hz, cfg.filter, cfg.filter_cutoff or None, cfg.filter_order,
                                             cfg.filter_zero_phase)
                stream_filter.window_settings = {"hz": cfg.hz, "window_sec": cfg.window_sec, "overlap": cfg.overlap}
            raw = raw_to_table(cfg.raw, hz=cfg.hz, window_sec=cfg.window_sec, overlap=cfg.overlap, device=dev,
                               ctx=ctx, rocket=cfg.rocket or None, samples=cfg.encoding == "raw", filter=stream_filter)
            log.print(f"Raw stream {cfg.raw}: {raw.count()} windows of {int(round(cfg.hz * cfg.window_sec))} "
                      f"samples ({cfg.window_sec:g} s at {cfg.hz:g} Hz, overlap {cfg.overlap:g})")
            if stream_filter is not None:
                log.print(f"Samples conditioned by {stream_filter}")
        else:
            raw = read_csv(cfg.data, device=dev if (cfg.csv_device and dev.type == "cuda") else None)
    # the HMM smoother's sequence keys, taken before the feature pipeline prunes the column
    seq_col = raw[cfg.hmm_sequence_col] if (cfg.hmm and cfg.hmm_sequence_col in raw) else None
    with timer.phase("feature_pipeline"):
        data, pipe_model, df = wisdm.prepare(raw, cfg.encoding)
    section(log, "Data Schema")
    log.print(data.print_schema(), end="")
    section(log, "Sample Data")
    log.print(data.show(5), end="")
    section(log, "Activity Count")
    log.print(data.group_count("activity").show(), end="")
    numeric_features = [n for n, t in data.dtypes if t in ("double", "int")]
    section(log, "Summary")
    log.print(describe_text(data.describe(numeric_features)))

    log.print(BANNER_PIPELINE)
    cols = data.columns
    df = df.select(["label", "features"] + cols)
    section(log, "Model Pipeline Schema")
    log.print(df.print_schema(), end="")
    section(log, "Sample Feature Data")
    import pandas as pd

    head = df.head(5)
    log.print(pd.DataFrame({c: [tuple(np.round(v[:9], 2)) if head[c].kind == "vector" else v
                                for v in head[c].data] for c in head.columns}))

    with timer.phase("random_split"):
        train, test = random_split(df, cfg.split, seed=cfg.seed)
    log.print(BANNER_TRAIN)
    log.print("Training Dataset Count : " + str(train.count()))
    log.print("Test Dataset Count     : " + str(test.count()))
    keep = [c for c in test.columns if c not in wisdm.MINIMIZED_VIEW]
    log.print(train.select(keep).show(5), end="")
    log.print(test.select(keep).show(5), end="")
    test_data = test.select([c for c in test.columns if c not in wisdm.SKIPPED_FOR_TEST])
    log.print(test_data.show(5), end="")

    if dev.type == "cuda":
        with timer.phase("device_warmup"):
            suite_names = [c for c in cfg.classifiers if c not in ("gbt", "knn", "ridge", "dtw")]
            if suite_names:
                warm_up_device(dev, train, cfg, classifiers=suite_names, test=test_data)
            if "gbt" in cfg.classifiers:  # the GBT kernels' code objects, on 256 rows and 2 rounds
                small = train.head(min(256, train.count()))
                est = make_estimator("gbt", cfg, dev, n_feature_columns(small), len(train["label"].meta["vocab"]))
                est.maxIter = 2
                wm = est.fit(small)
                wm.predict_all(wm.features_input(test_data))
                device_sync(dev)
            if "knn" in cfg.classifiers:  # the kNN kernels' code objects, on 256 rows (plain and grouped search)
                small = train.head(min(256, train.count()))
                est = make_estimator("knn", cfg, dev, n_feature_columns(small), len(train["label"].meta["vocab"]))
                est.fit(small).predict_all(features_tensor(test_data, "features", dev))
                est.leave_group_out(small)
                device_sync(dev)
            if "dtw" in cfg.classifiers:  # the DTW kernels' code objects, on 64 windows (plain and grouped search)
                small = train.head(min(64, train.count()))
                est = make_estimator("dtw", cfg, dev, n_feature_columns(small), len(train["label"].meta["vocab"]))
                est.fit(small).predict_all(features_tensor(test_data.head(min(64, test_data.count())), "features", dev))
                est.leave_group_out(small)
                device_sync(dev)
            if "ridge" in cfg.classifiers:  # the ridge kernels' code objects, on 256 rows, two folds and two alphas
                small = train.head(min(256, train.count()))
                est = make_estimator("ridge", cfg, dev, n_feature_columns(small), len(train["label"].meta["vocab"]))
                est.alphas, est.numFolds = est.alphas[:2], min(2, est.numFolds)
                est.fit(small).predict_all(features_tensor(test_data, "features", dev))
                device_sync(dev)
            if cfg.kmeans:  # the K-means / silhouette code objects, on 256 rows and 2 iterations
                from har.evaluation.evaluators import ClusteringEvaluator
                from har.models.kmeans import KMeans, kmeans_feature_cols, table_features

                Xs = table_features(train.head(min(256, train.count())), kmeans_feature_cols(cfg.encoding), dev)
                wk = KMeans(k=min(cfg.kmeans, Xs.shape[0]), maxIter=2, initMode=cfg.kmeans_init, seed=cfg.seed,
                            device=dev).fit_features(Xs)
                ClusteringEvaluator(device=dev).evaluate_tensors(Xs, wk.predict(Xs), wk.k)
                device_sync(dev)
            if cfg.gmm:  # the mixture (and its k-means init / silhouette) code objects, on 256 rows and 2 iterations
                from har.evaluation.evaluators import ClusteringEvaluator
                from har.models.gmm import GaussianMixture
                from har.models.kmeans import kmeans_feature_cols, table_features

                Xs = table_features(train.head(min(256, train.count())), kmeans_feature_cols(cfg.encoding), dev)
                wg = GaussianMixture(k=min(cfg.gmm, Xs.shape[0]), maxIter=2, covarianceType=cfg.gmm_cov,
                                     initMode=cfg.gmm_init, seed=cfg.seed, device=dev).fit_tensors(Xs)
                wg.score_samples(Xs)
                ClusteringEvaluator(device=dev).evaluate_tensors(Xs, wg.predict(Xs), wg.k)
                device_sync(dev)
        # not part of any "trained in" time below (the reference's timers exclude SparkContext start-up too)
        log.print("Device warm-up (HIP code objects, allocator) %.6f seconds" % timer.get("device_warmup"))
    log.print(BANNER_CLASSIFY)
    n_features = n_feature_columns(df)
    vocab = df["label"].meta["vocab"]
    n_classes = len(vocab)
    plain_rows, cv_rows, records = [], [], {}
    X_test = features_tensor(test_data, "features", dev)
    y_test = torch.as_tensor(test_data["label"].data.astype(np.int64), device=dev)
    smoother = test_offsets = None
    if cfg.hmm:  # transitions of the training rows in table order; the test rows keep their table order too
        from har.data.split import split_ids
        from har.models.hmm import HMMSmoother, offsets_of_keys
        from har.ops.hmm import count_segments

        ids = split_ids(df.count(), cfg.split, cfg.seed)  # the partition random_split made above

        def seq_offsets(bucket, n):
            if seq_col is None:
                return torch.tensor([0, n], dtype=torch.int64)
            return offsets_of_keys(seq_col.take_rows(np.nonzero(ids == bucket)[0]))

        hmm_est = HMMSmoother(sequenceCol=cfg.hmm_sequence_col, labelCol="label", emission=cfg.hmm_emission,
                              numClasses=n_classes, device=dev)
        with timer.phase("fit:hmm"):
            smoother = hmm_est.fit_labels(torch.as_tensor(train["label"].data.astype(np.int64)),
                                          seq_offsets(0, train.count()), n_classes)
        test_offsets = seq_offsets(1, test.count())
    em_pending = smoother is not None and cfg.hmm_em_iter > 0
    for name in cfg.classifiers:
        est = make_estimator(name, cfg, dev, n_features, n_classes)
        with timer.phase(f"fit:{name}"), data_parallel(ctx):
            model = est.fit(train)
        train_s = round(timer.get(f"fit:{name}"), 6)  # us resolution: sub-ms fits do not print as 0
        best = model.bestModel if hasattr(model, "bestModel") else model
        # the model's own input layout of the test rows (LR: the cached one-hot index + dense matrix,
        # trees / NB / MLP: the dense device matrix), prepared outside the timer like the table itself
        X_in = best.features_input(test_data) if hasattr(best, "features_input") else X_test
        with timer.phase(f"predict:{name}"):
            raw_pred, prob, pred = best.predict_all(X_in)
        test_s = round(timer.get(f"predict:{name}"), 6)
        label = str(model) + (" for Logistic Regression" if name == "lrcv" else "")
        model_header(log, label, train_s, test_s)
        preds = model.transform(test_data)
        show_class = 5 if name == "lr" else 0
        pv = preds.filter(preds["prediction"].data == show_class).select(
            ["UID", "probability", "label", "prediction"]).order_by("probability", ascending=False)
        log.print(pv.show(n=5, truncate=30), end="")
        with timer.phase(f"evaluate:{name}"):
            r = evaluate_all(y_test, pred, raw_pred, n_classes)
        evaluation_block(log, r)
        hmm_rec = {}
        if name == "knn" and cfg.knn_group_col:  # one grouped search of the training table against itself
            with timer.phase("leave_group_out:knn"):
                lgo = est.leave_group_out(train, cfg.knn_group_col)
                y_tr = torch.as_tensor(train["label"].data.astype(np.int64), device=lgo.device)
                hmm_rec["leave_group_out_accuracy"] = float((lgo == y_tr).double().mean())
            hmm_rec["leave_group_out_groups"] = int(len(np.unique(np.asarray(train[cfg.knn_group_col].data))))
            log.print("Leave-one-%s-out Accuracy = %g  (%d groups, %d training rows)"
                      % (cfg.knn_group_col, hmm_rec["leave_group_out_accuracy"], hmm_rec["leave_group_out_groups"],
                         train.count()))
        if name == "dtw" and cfg.dtw_group_col:  # one grouped search of the training table against itself
            with timer.phase("leave_group_out:dtw"):
                lgo = est.leave_group_out(train, cfg.dtw_group_col)
                y_tr = torch.as_tensor(train["label"].data.astype(np.int64), device=lgo.device)
                hmm_rec["leave_group_out_accuracy"] = float((lgo == y_tr).double().mean())
            hmm_rec["leave_group_out_groups"] = int(len(np.unique(np.asarray(train[cfg.dtw_group_col].data))))
            log.print("Leave-one-%s-out Accuracy = %g  (%d groups, %d training rows)"
                      % (cfg.dtw_group_col, hmm_rec["leave_group_out_accuracy"], hmm_rec["leave_group_out_groups"],
                         train.count()))
        if name == "dtw":  # predict.py --raw rebuilds the sample columns with these window settings
            best.raw_settings = {"hz": cfg.hz, "window_sec": cfg.window_sec, "overlap": cfg.overlap}
        if em_pending:  # Baum-Welch on the first fitted classifier's probabilities of the training rows
            em_pending = False
            hmm_est.emIter = cfg.hmm_em_iter
            X_tr = best.features_input(train) if hasattr(best, "features_input") else features_tensor(train, "features", dev)
            with timer.phase("fit:hmm-em"):
                smoother = hmm_est.fit_em(smoother, best.predict_all(X_tr)[1], seq_offsets(0, train.count()))
            h = smoother.objectiveHistory
            log.print("HMM Baum-Welch on %s: %d iterations, penalised objective %g -> %g"
                      % (name, smoother.emIterations, h[0], h[-1]))
        if smoother is not None:
            with timer.phase(f"smooth:{name}"):
                path, _ = smoother.decode(prob, test_offsets)
            hmm_rec = {"smoothed_accuracy": float((path.long() == y_test).double().mean()),
                       "segments": count_segments(path, test_offsets),
                       "raw_segments": count_segments(pred.to(torch.int32), test_offsets)}
            log.print("HMM smoothed Accuracy = %g  (%d segments, %d before smoothing; %d sequences)"
                      % (hmm_rec["smoothed_accuracy"], hmm_rec["segments"], hmm_rec["raw_segments"],
                         test_offsets.numel() - 1))
            if cfg.hmm_posterior:
                from har.ops.hmm import _lowest_argmax

                with timer.phase(f"posterior:{name}"):
                    gamma, loglik = smoother.posterior(prob, test_offsets)
                hmm_rec["posterior_accuracy"] = float((_lowest_argmax(gamma, 1)[1] == y_test).double().mean())
                hmm_rec["posterior_log_likelihood"] = float(loglik.sum())
                log.print("HMM posterior Accuracy = %g  (log-likelihood %g)"
                          % (hmm_rec["posterior_accuracy"], hmm_rec["posterior_log_likelihood"]))
        row = (csvout.cv_row if name.endswith("cv") else csvout.plain_row)(str(model), r, train_s, test_s)
        (cv_rows if name.endswith("cv") else plain_rows).append(row)
        records[name] = {"model": str(model), "train_s": train_s, "predict_s": test_s,
                         "train_windows_per_s": train.count() / max(train_s, 1e-9),
                         "predict_windows_per_s": test.count() / max(test_s, 1e-9), **r.as_dict(), **hmm_rec}
        if cfg.save_models and main_rank:
            persist.save(model, os.path.join(cfg.save_models, name), labels=vocab)
    kmeans_rec = None
    if cfg.kmeans:
        kmeans_rec = run_kmeans(cfg, dev, ctx, train, test, vocab, timer, log, main_rank)
    gmm_rec = None
    if cfg.gmm:
        gmm_rec = run_gmm(cfg, dev, train, test, vocab, timer, log, main_rank)
    if cfg.save_models and main_rank:
        persist.save(pipe_model, os.path.join(cfg.save_models, "pipeline"), labels=vocab)
        if getattr(raw, "rocket_model", None) is not None:  # predict.py --raw featurizes with the same transform
            persist.save(raw.rocket_model, os.path.join(cfg.save_models, "rocket"))
        if stream_filter is not None:  # predict.py --raw conditions the samples with the same sections
            persist.save(stream_filter, os.path.join(cfg.save_models, "filter"))
        if smoother is not None:
            persist.save(smoother, os.path.join(cfg.save_models, "hmm"), labels=vocab)
    world = ctx.world_size if ctx is not None else 1
    if not main_rank:
        log.close()
        return {"device": str(dev), "world_size": world, "models": records}

    if plain_rows:
        csvout.write_rows(os.path.join(cfg.out_dir, "additional_param.csv"), csvout.PLAIN_FIELDS, plain_rows,
                          append=cfg.append_csv)
    if cv_rows:
        csvout.write_rows(os.path.join(cfg.out_dir, "crossFold_additional_param.csv"), csvout.CV_FIELDS, cv_rows,
                          append=cfg.append_csv)
    summary = {"device": str(dev), "world_size": world, "encoding": cfg.encoding, "n_train": train.count(), "n_test": test.count(),
               "seed": cfg.seed, "wall_s": time.perf_counter() - t_run, "models": records,
               "phases_s": {k: round(v, 6) for k, v in timer.as_dict().items()}}
    if kmeans_rec is not None:
        summary["kmeans"] = kmeans_rec
    if gmm_rec is not None:
        summary["gmm"] = gmm_rec
    csvout.append_jsonl(os.path.join(cfg.out_dir, "metrics.jsonl"), summary)
    log.close()
    if cfg.report:
        from har.report.summary import write_report

        with open(os.path.join(cfg.out_dir, "result.txt")) as fh:
            write_report(summary, os.path.join(cfg.out_dir, "report"), fh.read())
    if cfg.plots:
        from har.report.plots import write_plots

        write_plots(data, numeric_features, cfg.plot_dir, seed=cfg.seed)
    return summary


def main(argv=None):
    cfg = config_from_args(argv)
    ctx = None
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:  # launched by torch.distributed.run: one rank per GPU
        ctx = hdist.init(device=None if cfg.device == "auto" else cfg.device)
    summary = run(cfg, ctx)
    from har.ops.logreg import solver_cache_clear

    solver_cache_clear()  # the run's tables are dropped: release the cached LR solvers' device memory
    if ctx is not None:
        hdist.shutdown(ctx)
        if not ctx.is_main:
            return
    print(json.dumps({k: {kk: (round(vv, 6) if isinstance(vv, float) else vv) for kk, vv in v.items()
                          if kk in ("accuracy", "f1", "train_s", "predict_s")} for k, v in summary["models"].items()}))


if __name__ == "__main__":
    main()

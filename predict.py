#!/usr/bin/env python3
"""``predict.py`` — batch inference / serving from saved models.

The reference never persists a model and its "Prediction made in" timer measures
only Spark's lazy query-plan construction (``Main/main.py:121-123``),
so it has no inference path to compare against.  This entry point closes that gap:
it loads the ``PipelineModel`` (encoder vocabularies) and any classifier written by
``main.py --save-models DIR`` (saved-model format: SURVEY.md §7.6), encodes raw CSV
rows exactly as at training time, predicts on the device and reports inference
throughput with device-synchronized timers.

    python main.py --preset all-numeric --save-models models/
    python predict.py --models models/ --model rf --data new_windows.csv --out preds.csv
    python predict.py --models models/ --model mlp --data wisdm_data.csv --csv-device --repeat 20
    python predict.py --models models/ --model rf --smooth hmm --segments-out timeline.csv --out preds.csv
    python predict.py --models models/ --model lr --raw raw.csv --out preds.csv    # after main.py --raw .. --preset rocket
    python predict.py --models models/ --model ridge --raw raw.csv --out preds.csv # after main.py --raw .. --preset rocket-ridge
    python predict.py --models models/ --model dtw --raw raw.csv --out preds.csv   # after main.py --raw .. --preset dtw

Output CSV columns: ``row, UID (if present), prediction, label_name, probability``.
``--smooth hmm`` (needs ``<models>/hmm``, written by ``main.py --hmm --save-models``) decodes the
predictions of every sequence (runs of equal ``--sequence-col`` values, in row order) with the saved
HMMSmoother: the CSV gains ``smoothed_prediction, smoothed_label_name``, the JSON record ``smooth_s``,
``segments`` (and ``smoothed_accuracy`` for labelled input), and ``--segments-out FILE`` writes the
timeline ``sequence, first_row, last_row, state, label_name``.  ``--smooth hmm-posterior`` labels every
window with the argmax of its forward-backward posterior instead: the CSV also gains
``smoothed_confidence`` (that posterior's maximum) and the JSON ``smoothed_log_likelihood``.
When the input still has the ``ACTIVITY`` column the script also prints the
reference's evaluation block (accuracy, weighted F1, ...).  Rows whose string
categories were never seen at training time are rejected by the indexers unless
``--handle-invalid keep`` (Spark's ``handleInvalid`` semantics).
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from har.config import DEFAULT_WISDM  # noqa: E402
from har.data.csv_io import read_csv  # noqa: E402
from har.features.encode import StringIndexerModel  # noqa: E402
from har.models.base import features_tensor, resolve_device  # noqa: E402
from har.utils import persist  # noqa: E402
from har.utils.timing import device_sync  # noqa: E402


def encode(pipeline, table, handle_invalid: str = "error"):
    """Apply the fitted pipeline; a label indexer whose input column is absent (unlabeled
    serving data) is skipped."""
    for st in pipeline.stages:
        if isinstance(st, StringIndexerModel):
            if st.inputCol not in table.columns:
                continue
            if handle_invalid != "error":
                st.handleInvalid = handle_invalid
        table = st.transform(table)
    return table


def run(args) -> dict:
    dev = resolve_device(None if args.device == "auto" else args.device)
    pipe = persist.load(os.path.join(args.models, "pipeline"), device=dev)
    model = persist.load(os.path.join(args.models, args.model), device=dev)
    with open(os.path.join(args.models, args.model, "metadata.json")) as f:
        labels = json.load(f).get("labels")
    model = getattr(model, "bestModel", model)
    smoother = None
    if args.smooth:
        if args.smooth not in ("hmm", "hmm-posterior"):
            raise ValueError(f"unknown smoother {args.smooth!r} (hmm | hmm-posterior)")
        smoother = persist.load(os.path.join(args.models, "hmm"), device=dev)
    t0 = time.perf_counter()
    if args.raw:  # raw sensor rows: the saved window settings and rocket transform, then the saved pipeline
        from har.features.raw import raw_to_table

        rdir = os.path.join(args.models, "rocket")
        fdir = os.path.join(args.models, "filter")
        # the samples are conditioned as at training time when main.py --filter saved its sections
        flt = persist.load(fdir, device=dev) if os.path.isdir(fdir) else None
        rs = getattr(model, "raw_settings", None)
        if rs is not None:  # a DTW model: the windows' own samples, with the saved window settings
            raw = raw_to_table(args.raw, hz=rs["hz"], window_sec=rs["window_sec"], overlap=rs["overlap"], device=dev,
                               samples=True, filter=flt)
        elif flt is not None and not os.path.isdir(rdir):  # the WISDM columns of the filtered stream
            ws = flt.window_settings or {"hz": flt.hz, "window_sec": 10.0, "overlap": 0.0}
            raw = raw_to_table(args.raw, hz=ws["hz"], window_sec=ws["window_sec"], overlap=ws["overlap"], device=dev,
                               filter=flt)
        elif not os.path.isdir(rdir):
            raise FileNotFoundError(f"--raw needs the saved featurizer {rdir}: write it with "
                                    "main.py --raw PATH --rocket N --save-models DIR")
        else:
            rk = persist.load(rdir, device=dev)
            raw = raw_to_table(args.raw, hz=rk.hz, window_sec=rk.window / rk.hz, overlap=1.0 - rk.stride / rk.window,
                               device=dev, rocket=rk, filter=flt)
    else:
        raw = read_csv(args.data, device=dev if (args.csv_device and dev.type == "cuda") else None)
    table = encode(pipe, raw, args.handle_invalid)
    if type(model).__name__ == "KMeansModel":
        return run_kmeans(args, model, table, labels, dev, t0)
    if type(model).__name__ == "GaussianMixtureModel":
        return run_gmm(args, model, table, labels, dev, t0)
    X = features_tensor(table, "features", dev)
    device_sync(dev)
    t_ingest = time.perf_counter() - t0
    out = model.predict_all(X)  # warm-up (code objects, allocator)
    device_sync(dev)
    t1 = time.perf_counter()
    for _ in range(args.repeat):
        out = model.predict_all(X)
    device_sync(dev)
    t_pred = (time.perf_counter() - t1) / max(1, args.repeat)
    raw_pred, prob, pred = out
    n = X.shape[0]
    rec = {"model": str(model), "rows": n, "device": str(dev), "ingest_encode_s": round(t_ingest, 6),
           "predict_s": round(t_pred, 6), "predict_windows_per_s": n / max(t_pred, 1e-12)}
    if "label" in table.columns:
        from har.evaluation.evaluators import evaluate_all

        y = torch.as_tensor(table["label"].data.astype(np.int64), device=dev)
        r = evaluate_all(y, pred, raw_pred, int(raw_pred.shape[1]))
        rec.update({"accuracy": r.accuracy, "f1": r.f1})
    sp = conf = None
    if smoother is not None:
        from har.models.hmm import sequence_offsets
        from har.ops.hmm import segments

        if table.count() != raw.count():
            raise ValueError("--smooth needs every input row (no --handle-invalid skip): the sequences are runs of rows")
        offsets = sequence_offsets(raw, args.sequence_col or smoother.sequenceCol)
        device_sync(dev)
        t2 = time.perf_counter()
        if args.smooth == "hmm-posterior":  # the smoothed probability of every window; its argmax is the label
            from har.ops.hmm import _lowest_argmax

            gamma, loglik = smoother.posterior(prob, offsets)
            top, path = _lowest_argmax(gamma, 1)
            path = path.to(torch.int32)
        else:
            path, _ = smoother.decode(prob, offsets)
        device_sync(dev)
        rec["smooth_s"] = round(time.perf_counter() - t2, 6)
        if args.smooth == "hmm-posterior":
            rec["smoothed_log_likelihood"] = float(loglik.sum())
            conf = top.cpu().numpy()
        segs = segments(path, offsets)
        rec["segments"] = len(segs)
        sp = path.long().cpu().numpy()
        if "label" in table.columns:
            rec["smoothed_accuracy"] = float((sp == table["label"].data.astype(np.int64)).mean())
        if args.segments_out:
            with open(args.segments_out, "w", newline="") as f:
                w = csv.writer(f)
                w.writerow(["sequence", "first_row", "last_row", "state", "label_name"])
                for q, a, b, k in segs:
                    w.writerow([q, a, b, k, labels[k] if labels and k < len(labels) else ""])
    if args.out:
        p = pred.long().cpu().numpy()
        pr = prob.float().cpu().numpy()
        uid = table["UID"].data if "UID" in table.columns else None
        with open(args.out, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["row"] + (["UID"] if uid is not None else []) + ["prediction", "label_name", "probability"]
                       + (["smoothed_prediction", "smoothed_label_name"] if sp is not None else [])
                       + (["smoothed_confidence"] if conf is not None else []))
            for i in range(n):
                name = labels[p[i]] if labels and p[i] < len(labels) else ""
                extra = []
                if sp is not None:
                    extra = [int(sp[i]), labels[sp[i]] if labels and sp[i] < len(labels) else ""]
                if conf is not None:
                    extra.append(float(conf[i]))
                w.writerow([i] + ([int(uid[i])] if uid is not None else []) + [int(p[i]), name, float(pr[i, p[i]])] + extra)
    return rec


def run_kmeans(args, model, table, labels, dev, t0) -> dict:
    """``--model kmeans``: the cluster id per row and, when the saved model carries a label map, the
    majority label of that cluster."""
    from har.models.kmeans import table_features

    X = table_features(table, model.feature_cols, dev)
    device_sync(dev)
    t_ingest = time.perf_counter() - t0
    pred = model.predict(X)  # warm-up (code objects, allocator)
    device_sync(dev)
    t1 = time.perf_counter()
    for _ in range(args.repeat):
        pred = model.predict(X)
    device_sync(dev)
    t_pred = (time.perf_counter() - t1) / max(1, args.repeat)
    n = X.shape[0]
    rec = {"model": str(model), "rows": n, "device": str(dev), "ingest_encode_s": round(t_ingest, 6),
           "predict_s": round(t_pred, 6), "predict_windows_per_s": n / max(t_pred, 1e-12),
           "clusters_used": int(torch.unique(pred).numel())}
    maj = model.majority_labels
    if maj is not None and "label" in table.columns:
        y = torch.as_tensor(table["label"].data.astype(np.int64), device=dev)
        rec["majority_label_accuracy"] = float((torch.as_tensor(maj, device=dev)[pred] == y).double().mean())
    if args.out:
        p = pred.long().cpu().numpy()
        uid = table["UID"].data if "UID" in table.columns else None
        with open(args.out, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["row"] + (["UID"] if uid is not None else []) + ["cluster"]
                       + (["majority_label", "label_name"] if maj is not None else []))
            for i in range(n):
                extra = []
                if maj is not None:
                    k = maj[p[i]]
                    extra = [k, labels[k] if labels and k < len(labels) else ""]
                w.writerow([i] + ([int(uid[i])] if uid is not None else []) + [int(p[i])] + extra)
    return rec


def run_gmm(args, model, table, labels, dev, t0) -> dict:
    """``--model gmm``: the cluster id per row, its majority label when the saved model carries a label map,
    the largest probability and the row's log-likelihood."""
    from har.models.kmeans import table_features

    X = table_features(table, model.feature_cols, dev)
    device_sync(dev)
    t_ingest = time.perf_counter() - t0
    e = model._estep(X)  # warm-up (code objects, allocator)
    device_sync(dev)
    t1 = time.perf_counter()
    for _ in range(args.repeat):
        e = model._estep(X)
    device_sync(dev)
    t_pred = (time.perf_counter() - t1) / max(1, args.repeat)
    n = X.shape[0]
    pred = e.pred.long()
    ll = model.score_samples(X)
    rec = {"model": str(model), "rows": n, "device": str(dev), "ingest_encode_s": round(t_ingest, 6),
           "predict_s": round(t_pred, 6), "predict_windows_per_s": n / max(t_pred, 1e-12),
           "clusters_used": int(torch.unique(pred).numel()), "mean_log_likelihood": float(ll.mean()) if n else 0.0}
    maj = model.majority_labels
    if maj is not None and "label" in table.columns:
        y = torch.as_tensor(table["label"].data.astype(np.int64), device=dev)
        rec["majority_label_accuracy"] = float((torch.as_tensor(maj, device=dev)[pred] == y).double().mean())
    if args.out:
        p = pred.cpu().numpy()
        top = e.resp.max(dim=1).values.cpu().numpy() if n else np.zeros(0)
        lls = ll.cpu().numpy()
        uid = table["UID"].data if "UID" in table.columns else None
        with open(args.out, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["row"] + (["UID"] if uid is not None else []) + ["cluster"]
                       + (["majority_label", "label_name"] if maj is not None else []) + ["probability", "log_likelihood"])
            for i in range(n):
                extra = []
                if maj is not None:
                    k = maj[p[i]]
                    extra = [k, labels[k] if labels and k < len(labels) else ""]
                w.writerow([i] + ([int(uid[i])] if uid is not None else []) + [int(p[i])] + extra
                           + [float(top[i]), float(lls[i])])
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description="Batch inference from models saved by main.py --save-models")
    ap.add_argument("--models", required=True, help="directory written by main.py --save-models")
    ap.add_argument("--model", default="rf", help="sub-directory name: lr, lrcv, dt, dtcv, rf, rfcv, nb, mlp, gbt, knn, ridge, dtw, kmeans, gmm")
    ap.add_argument("--data", default=DEFAULT_WISDM)
    ap.add_argument("--raw", default="", help="raw user,activity,timestamp,x,y,z rows instead of --data: windowed and "
                                              "featurized with the saved settings and <models>/rocket")
    ap.add_argument("--out", default="")
    ap.add_argument("--device", default="auto")
    ap.add_argument("--csv-device", action="store_true", help="parse the CSV with the HIP kernels")
    ap.add_argument("--repeat", type=int, default=1, help="timed prediction passes (throughput)")
    ap.add_argument("--handle-invalid", default="error", choices=["error", "skip", "keep"])
    ap.add_argument("--smooth", default="", help="hmm: Viterbi-smooth the predictions with <models>/hmm; "
                                                 "hmm-posterior: forward-backward posteriors and their argmax")
    ap.add_argument("--sequence-col", default="", help="column whose runs are the sequences (default: the saved one)")
    ap.add_argument("--segments-out", default="", help="with --smooth: write the timeline's segments to this CSV")
    rec = run(ap.parse_args(argv))
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main()

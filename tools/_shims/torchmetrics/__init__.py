"""Authoring-container stub: the reference's utils/eval_utils.py imports torchmetrics at module scope (no name from it is used by
the metric classes that tools/make_golden_metrics.py runs)."""

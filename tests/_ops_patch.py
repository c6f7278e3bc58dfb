"""Replacing a wrapper of the ops package for the length of a test."""
import sys

from pcc_geo_cnn_v2_amd import ops


def patch_ops(monkeypatch, name, replacement):
    """monkeypatch.setattr for `ops.<name>`: callers outside the package read the package's attribute, callers inside it the defining
    module's, so both are replaced (and both restored by monkeypatch.undo())."""
    home = sys.modules[getattr(ops, name).__module__]
    monkeypatch.setattr(ops, name, replacement)
    monkeypatch.setattr(home, name, replacement)

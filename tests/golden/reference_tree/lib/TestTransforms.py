"""Placeholder for the reference's lib/TestTransforms.py (test.py:16)."""

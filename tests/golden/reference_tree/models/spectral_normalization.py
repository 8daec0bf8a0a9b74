"""Placeholder for the reference's models/spectral_normalization.py."""

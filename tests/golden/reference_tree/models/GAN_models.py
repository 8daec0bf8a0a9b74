"""Placeholder for the reference's models/GAN_models.py."""

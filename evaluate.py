"""Drop-in launcher: ``python evaluate.py --step_ckpt ... `` (the reference's ``test.py``)."""
from ucd_amd.evaluate import cli

if __name__ == "__main__":
    cli()

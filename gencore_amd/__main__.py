"""`python -m gencore_amd`: the gencore command line (gencore_amd/cli.py)."""
import sys

from .cli import main

sys.exit(main())

"""python -m panfeed_amd ...: the panfeed command (cli.main)"""
import sys

from .cli import main

if __name__ == "__main__":
    sys.exit(main())

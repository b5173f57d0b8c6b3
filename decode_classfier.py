"""`python decode_classfier.py --task dna --guidance_scale 1.5` — same entry point name as the reference's decode_classfier.py;
the implementation is svdd_amd/cli.py (method "classfier")."""
from svdd_amd.cli import main

if __name__ == "__main__":
    main("classfier")

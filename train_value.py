"""`python train_value.py --task dna --cdq --iters 100` - trains the value function that the guided samplers take (Monte-Carlo
regression, or CD-Q with --cdq; reference Enformer.BaseModel.forward, Enformer.py:163-267); the implementation is
svdd_amd/cli.py (train_value)."""
from svdd_amd.cli import main_train

if __name__ == "__main__":
    main_train()

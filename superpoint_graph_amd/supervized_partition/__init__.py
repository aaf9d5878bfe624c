"""The learned (supervised) partition's loss side with the reference's names (supervized_partition/losses.py)."""

"""`wenet.bin.align_wav:main`: forced alignment of a transcript (the job of the reference's `wenet/bin/alignment.py`)."""
from reverb_amd.bin.align_wav import get_args, main  # noqa: F401

if __name__ == "__main__":
    main()

"""``src.prepare_data``: rank-normalise a raw characteristic panel into an ordinary ``data_dir``."""
from deeplearninginassetpricing_paperreplication_amd.data.transforms import (  # noqa: F401
    main, prepare_data_dir, prepare_split, rank_characteristics, rank_characteristics_numpy, row_filter)

if __name__ == "__main__":
    main()

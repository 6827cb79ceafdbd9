from .prn_data import DevicePRNBatcher, PRNDeviceLoader, PRNSampleSet  # noqa: F401
